"""ctypes binding of the C-ABI in include/farnn.h (libfarnn_hip.so).

There is no CPU fallback: if the shared library has not been built (``__graft_entry__.build()``
or ``python -m re2nn_seq_amd.csrc.build``) or no MI355X is visible, the functions here raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FARNN_LIB: a diagnostic build of the same library (csrc/build.py --probes); never a different implementation
LIB_PATH = os.environ.get('FARNN_LIB') or os.path.join(_HERE, 'csrc', 'libfarnn_hip.so')

OK = 0
NL = {'none': 0, 'relu': 1, 'tanh': 2, 'relutanh': 3, 'sigmoid': 4}
SEMIRING = {'sum': 0, 'max': 1}
MODE_LOCAL, MODE_FULL, MODE_RE = 0, 1, 2
HOST_SLOTS = 4                  # FARNN_HOST_SLOTS: batches the host-buffer path keeps in flight
KERN_CHAIN, KERN_SCORE, KERN_PREP, KERN_TABLE = 0, 1, 2, 3

_f32p = C.POINTER(C.c_float)


class FarnnError(RuntimeError):
    pass


class OnehotIfstDesc(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('C', C.c_int32),
                ('T', _f32p), ('W', _f32p), ('O', _f32p), ('h0', _f32p), ('hT', _f32p), ('P', _f32p),
                ('nl', C.c_int32), ('semiring', C.c_int32), ('threshold', C.c_float),
                ('o_idx', C.c_int32), ('use_crf', C.c_int32), ('crf_trans', _f32p),
                ('weights_on_device', C.c_int32)]


class OnehotFst4Desc(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('C', C.c_int32),
                ('T4', _f32p), ('W4', _f32p), ('h0', _f32p), ('hT', _f32p), ('P', _f32p),
                ('semiring', C.c_int32), ('threshold', C.c_float), ('o_idx', C.c_int32),
                ('weights_on_device', C.c_int32)]


class OnehotInd1Desc(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('C', C.c_int32),
                ('T', _f32p), ('W', _f32p), ('Oten', _f32p), ('h0', _f32p), ('hT', _f32p), ('P', _f32p),
                ('semiring', C.c_int32), ('mask_by_output', C.c_int32), ('threshold', C.c_float),
                ('o_idx', C.c_int32), ('weights_on_device', C.c_int32)]


class DecompIfstDesc(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('R', C.c_int32), ('K', C.c_int32),
                ('Vgen', _f32p), ('S1', _f32p), ('S2', _f32p), ('W', _f32p), ('Cout', _f32p),
                ('h0', _f32p), ('hT', _f32p), ('P', _f32p),
                ('farnn', C.c_int32),
                ('Wss1', _f32p), ('Wrs1', _f32p), ('bs1', _f32p),
                ('Wss2', _f32p), ('Wrs2', _f32p), ('bs2', _f32p),
                ('sigmoid_exponent', C.c_float), ('nl', C.c_int32), ('semiring', C.c_int32),
                ('threshold', C.c_float), ('o_idx', C.c_int32), ('use_crf', C.c_int32),
                ('crf_trans', _f32p), ('weights_on_device', C.c_int32)]


class VgenFold(C.Structure):
    _fields_ = [('V_embed', _f32p), ('E', _f32p), ('G', _f32p), ('beta', _f32p), ('D', C.c_int32), ('add_nl', C.c_int32),
                ('normalize', C.c_int32), ('on_device', C.c_int32)]


NORM = {'none': 0, 'l1': 1, 'l2': 2, 'l1-rank': 3, 'l2-rank': 4}


class DecompInd1Desc(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('R', C.c_int32), ('RO', C.c_int32), ('K', C.c_int32),
                ('Vgen', _f32p), ('S1', _f32p), ('S2', _f32p), ('W', _f32p), ('Cout', _f32p),
                ('S1o', _f32p), ('S2o', _f32p), ('Wo', _f32p),
                ('h0', _f32p), ('hT', _f32p), ('P', _f32p),
                ('farnn', C.c_int32),
                ('Wss1', _f32p), ('Wrs1', _f32p), ('bs1', _f32p),
                ('Wss2', _f32p), ('Wrs2', _f32p), ('bs2', _f32p),
                ('sigmoid_exponent', C.c_float), ('nl', C.c_int32), ('semiring', C.c_int32),
                ('threshold', C.c_float), ('o_idx', C.c_int32), ('use_crf', C.c_int32),
                ('crf_trans', _f32p), ('weights_on_device', C.c_int32)]


class EdgeList(C.Structure):
    _fields_ = [('n_edges', C.c_int64),
                ('word', C.POINTER(C.c_int32)), ('from_', C.POINTER(C.c_int32)), ('to', C.POINTER(C.c_int32)),
                ('label', C.POINTER(C.c_int32)), ('val', _f32p)]


class DecompFstDesc(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('R', C.c_int32), ('RW', C.c_int32), ('K', C.c_int32),
                ('Vgen', _f32p), ('C', _f32p), ('S1', _f32p), ('S2', _f32p), ('Cw', _f32p),
                ('S1w', _f32p), ('S2w', _f32p), ('WW', _f32p),
                ('h0', _f32p), ('hT', _f32p), ('P', _f32p),
                ('farnn', C.c_int32),
                ('Wss1', _f32p), ('Wrs1', _f32p), ('bs1', _f32p),
                ('Wss2', _f32p), ('Wrs2', _f32p), ('bs2', _f32p),
                ('sigmoid_exponent', C.c_float), ('nl', C.c_int32), ('semiring', C.c_int32),
                ('threshold', C.c_float), ('o_idx', C.c_int32), ('use_crf', C.c_int32),
                ('crf_trans', _f32p), ('weights_on_device', C.c_int32)]


# every symbol include/farnn.h declares, with its ctypes signature (tests check the exports)
_vp = C.c_void_p
class TrainDims(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('R', C.c_int32), ('K', C.c_int32), ('nl', C.c_int32),
                ('threshold', C.c_float), ('o_idx', C.c_int32), ('farnn', C.c_int32), ('sigmoid_exponent', C.c_float),
                ('use_crf', C.c_int32)]


class TrainWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('Vgen', 'S1', 'S2', 'W', 'C', 'h0', 'hT', 'P', 'crf_trans',
                                          'Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')]


class TrainOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('loss', 'dVgen', 'dS1', 'dS2', 'dW', 'dC', 'dh0', 'dhT', 'tags', 'dtrans',
                                          'dWss1', 'dWrs1', 'dbs1', 'dWss2', 'dWrs2', 'dbs2')]


class DecompFstTrainDims(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('R', C.c_int32), ('Q', C.c_int32), ('K', C.c_int32), ('nl', C.c_int32),
                ('threshold', C.c_float), ('o_idx', C.c_int32), ('farnn', C.c_int32), ('sigmoid_exponent', C.c_float),
                ('use_crf', C.c_int32)]


class DecompFstTrainWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('Vgen', 'Ce', 'S1', 'S2', 'Cw', 'S1w', 'S2w', 'WW', 'h0', 'hT', 'P', 'crf_trans',
                                          'Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')]


class DecompFstTrainOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('loss', 'dVgen', 'dCe', 'dS1', 'dS2', 'dCw', 'dS1w', 'dS2w', 'dWW', 'dh0', 'dhT', 'tags',
                                          'dtrans', 'dWss1', 'dWrs1', 'dbs1', 'dWss2', 'dWrs2', 'dbs2')]


class Teacher(C.Structure):
    _fields_ = [('mode', C.c_int32), ('c1', C.c_float), ('pi', C.c_float)]


TEACHER = {'kd': 1, 'pr': 2}      # FARNN_TEACHER_KD, FARNN_TEACHER_PR


class OnehotTrainDims(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('C', C.c_int32), ('nl', C.c_int32), ('threshold', C.c_float),
                ('o_idx', C.c_int32)]


class OnehotTrainWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('T', 'W', 'O', 'h0', 'hT', 'P')]


class OnehotTrainOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('loss', 'dT', 'tags')]


class Fst4TrainDims(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('C', C.c_int32), ('threshold', C.c_float), ('o_idx', C.c_int32)]


class Fst4TrainWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('T4', 'W4', 'h0', 'hT', 'P')]


class Fst4TrainOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('loss', 'dT4', 'dW4', 'tags')]


class Ind1TrainDims(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('C', C.c_int32), ('mask_by_output', C.c_int32),
                ('threshold', C.c_float), ('o_idx', C.c_int32)]


class Ind1TrainWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('T', 'W', 'O', 'h0', 'hT', 'P')]


class Ind1TrainOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('loss', 'dT', 'tags')]


class Decomp1TrainDims(C.Structure):
    _fields_ = [('V', C.c_int32), ('S', C.c_int32), ('R', C.c_int32), ('RO', C.c_int32), ('C', C.c_int32), ('nl', C.c_int32),
                ('threshold', C.c_float), ('o_idx', C.c_int32)]


class Decomp1TrainWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('Vgen', 'S1', 'S2', 'W', 'C', 'S1o', 'S2o', 'h0', 'hT', 'P')]


class Decomp1TrainOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('loss', 'dVgen', 'dS1', 'dS2', 'dW', 'dC', 'dS1o', 'dS2o', 'dh0', 'dhT', 'tags')]


class Decomp1GateWeights(C.Structure):
    _fields_ = [('farnn', C.c_int32)] + [(n, C.c_void_p) for n in ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')] + \
               [('sigmoid_exponent', C.c_float)]


class Decomp1GateOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('dWss1', 'dWrs1', 'dbs1', 'dWss2', 'dWrs2', 'dbs2')]


class OptimDesc(C.Structure):
    _fields_ = [('kind', C.c_int32), ('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double)]


class ScoreCounts(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ('n', 'same', 'canon_same', 'tp', 'fp', 'fn', 'pred_spans', 'gold_spans', 'matches',
                                         'errors', 'adds')] + [('loss_sum', C.c_double), ('per_type', C.POINTER(C.c_int64))]


SCORE_WAVES = 16                               # csrc/farnn_score.hip: sequences in flight (one per wavefront of the launch)
SCORE_TYPE_ROWS = 5                            # per_type rows: B- tags, B- labels, matches, first B- tag, first B- label

OPTIM_SGD, OPTIM_ADAM = 0, 1
OPTIM_CHUNK, OPTIM_MAX_TENSORS = 2048, 32      # csrc/optim.hip.h: elements per workgroup, tensors per launch

SIGNATURES = {
    'farnn_score_create': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int]),
    'farnn_score_destroy': (None, [C.c_void_p]),
    'farnn_score_add': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'farnn_score_read': (C.c_int, [C.c_void_p, C.POINTER(ScoreCounts), C.c_void_p]),
    'farnn_score_reset': (C.c_int, [C.c_void_p, C.c_void_p]),
    'farnn_cp_create': (C.c_int, [C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_double), C.c_int32, C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_cp_destroy': (None, [C.c_void_p]),
    'farnn_cp_mttkrp': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'farnn_cp_normal_matrix': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    'farnn_cp_solve': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'farnn_cp_run': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p]),
    'farnn_cp_set_profiling': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_cp_time': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'farnn_cp_norm2': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'farnn_cp_create_n': (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_double),
                                    C.c_int32, C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_cp_order': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    'farnn_cp_mttkrp_n': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    'farnn_cp_normal_matrix_n': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    'farnn_cp_run_n': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_void_p), C.POINTER(C.c_double),
                                 C.POINTER(C.c_int32), C.c_void_p]),
    'farnn_optim_create': (C.c_int, [C.POINTER(OptimDesc), C.POINTER(C.c_int64), C.c_int32, C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_optim_destroy': (None, [C.c_void_p]),
    'farnn_optim_step': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_void_p), C.c_void_p]),
    'farnn_optim_set_lr': (C.c_int, [C.c_void_p, C.c_double]),
    'farnn_optim_steps': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    'farnn_optim_set_steps': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    'farnn_onehot_train_create': (C.c_int, [C.POINTER(OnehotTrainDims), C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_onehot_train_destroy': (None, [C.c_void_p]),
    'farnn_onehot_ifst_train_step': (C.c_int, [C.c_void_p, C.POINTER(OnehotTrainWeights), C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                               C.POINTER(OnehotTrainOutputs), C.c_void_p]),
    'farnn_onehot_train_set_profiling': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_onehot_train_time': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'farnn_onehot_train_set_semiring': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_fst4_train_create': (C.c_int, [C.POINTER(Fst4TrainDims), C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_fst4_train_destroy': (None, [C.c_void_p]),
    'farnn_fst4_train_step': (C.c_int, [C.c_void_p, C.POINTER(Fst4TrainWeights), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                        C.POINTER(Fst4TrainOutputs), C.c_void_p]),
    'farnn_fst4_train_set_profiling': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_fst4_train_time': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'farnn_fst4_train_set_semiring': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_ind1_train_create': (C.c_int, [C.POINTER(Ind1TrainDims), C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_ind1_train_destroy': (None, [C.c_void_p]),
    'farnn_ind1_train_step': (C.c_int, [C.c_void_p, C.POINTER(Ind1TrainWeights), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                        C.POINTER(Ind1TrainOutputs), C.c_void_p]),
    'farnn_ind1_train_set_profiling': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_ind1_train_time': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'farnn_ind1_train_set_semiring': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_decomp_ind1_train_create': (C.c_int, [C.POINTER(Decomp1TrainDims), C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_decomp_ind1_train_destroy': (None, [C.c_void_p]),
    'farnn_decomp_ind1_train_step': (C.c_int, [C.c_void_p, C.POINTER(Decomp1TrainWeights), C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                               C.POINTER(Decomp1TrainOutputs), C.c_void_p]),
    'farnn_decomp_ind1_crf_train_step': (C.c_int, [C.c_void_p, C.POINTER(Decomp1TrainWeights), C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                                   C.POINTER(Decomp1TrainOutputs), C.c_void_p, C.c_void_p]),
    'farnn_decomp_ind1_gated_train_step': (C.c_int, [C.c_void_p, C.POINTER(Decomp1TrainWeights), C.POINTER(Decomp1GateWeights),
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                                     C.POINTER(Decomp1TrainOutputs), C.POINTER(Decomp1GateOutputs), C.c_void_p,
                                                     C.c_void_p]),
    'farnn_decomp_ind1_gated_max_train_step': (C.c_int, [C.c_void_p, C.POINTER(Decomp1TrainWeights), C.POINTER(Decomp1GateWeights),
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                                         C.POINTER(Decomp1TrainOutputs), C.POINTER(Decomp1GateOutputs), C.c_void_p,
                                                         C.c_void_p]),
    'farnn_decomp_ind1_train_set_profiling': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_decomp_ind1_train_time': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'farnn_decomp_ind1_train_set_semiring': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_decomp_fst_train_create': (C.c_int, [C.POINTER(DecompFstTrainDims), C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_decomp_fst_train_set_semiring': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_decomp_fst_train_destroy': (None, [C.c_void_p]),
    'farnn_decomp_fst_train_step': (C.c_int, [C.c_void_p, C.POINTER(DecompFstTrainWeights), C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                              C.POINTER(DecompFstTrainOutputs), C.c_void_p]),
    'farnn_decomp_fst_train_set_profiling': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_decomp_fst_train_time': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'farnn_train_create': (C.c_int, [C.POINTER(TrainDims), C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_train_destroy': (None, [C.c_void_p]),
    'farnn_decomp_ifst_train_step': (C.c_int, [C.c_void_p, C.POINTER(TrainWeights), C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                               C.POINTER(TrainOutputs), C.c_void_p]),
    'farnn_decomp_ifst_teacher_train_step': (C.c_int, [C.c_void_p, C.POINTER(TrainWeights), C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.POINTER(Teacher), C.c_int32, C.c_int32,
                                                       C.c_int64, C.POINTER(TrainOutputs), C.c_void_p]),
    'farnn_decomp_ifst_teacher_max_train_step': (C.c_int, [C.c_void_p, C.POINTER(TrainWeights), C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.POINTER(Teacher), C.c_int32, C.c_int32,
                                                           C.c_int64, C.POINTER(TrainOutputs), C.c_void_p]),
    'farnn_decomp_sf_train_create': (C.c_int, [C.POINTER(TrainDims), C.c_int, C.POINTER(C.c_void_p)]),
    'farnn_decomp_sf_train_step': (C.c_int, [C.c_void_p, C.POINTER(TrainWeights), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                             C.c_int32, C.c_int64, C.POINTER(TrainOutputs), C.c_void_p, C.c_void_p]),
    'farnn_train_set_profiling': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_train_time': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'farnn_train_set_semiring': (C.c_int, [C.c_void_p, C.c_int32]),
    'farnn_onehot_ifst_create': (C.c_int, [C.POINTER(OnehotIfstDesc), C.c_int, C.POINTER(_vp)]),
    'farnn_onehot_ifst_create_from_edges': (C.c_int, [C.POINTER(OnehotIfstDesc), C.POINTER(EdgeList), C.c_int,
                                                      C.POINTER(_vp)]),
    'farnn_onehot_ifst_create_compact': (C.c_int, [C.POINTER(OnehotIfstDesc), C.POINTER(EdgeList), C.c_int,
                                                   C.POINTER(_vp)]),
    'farnn_has_compact': (C.c_int, [_vp]),
    'farnn_set_compact': (C.c_int, [_vp, C.c_int32]),
    'farnn_onehot_fst4_create_from_edges': (C.c_int, [C.POINTER(OnehotFst4Desc), C.POINTER(EdgeList), C.c_int,
                                                      C.POINTER(_vp)]),
    'farnn_onehot_ind1_create_from_edges': (C.c_int, [C.POINTER(OnehotInd1Desc), C.POINTER(EdgeList), C.c_int,
                                                      C.POINTER(_vp)]),
    'farnn_onehot_fst4_create': (C.c_int, [C.POINTER(OnehotFst4Desc), C.c_int, C.POINTER(_vp)]),
    'farnn_onehot_ind1_create': (C.c_int, [C.POINTER(OnehotInd1Desc), C.c_int, C.POINTER(_vp)]),
    'farnn_decomp_ifst_create': (C.c_int, [C.POINTER(DecompIfstDesc), C.c_int, C.POINTER(_vp)]),
    'farnn_decomp_ifst_create_folded': (C.c_int, [C.POINTER(DecompIfstDesc), C.POINTER(VgenFold), C.c_int, C.POINTER(_vp)]),
    'farnn_decomp_ind1_create': (C.c_int, [C.POINTER(DecompInd1Desc), C.c_int, C.POINTER(_vp)]),
    'farnn_decomp_fst_create': (C.c_int, [C.POINTER(DecompFstDesc), C.c_int, C.POINTER(_vp)]),
    'farnn_tag': (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    'farnn_reserve': (C.c_int, [_vp, C.c_int32, C.c_int32]),
    'farnn_decomp_sf_create': (C.c_int, [C.POINTER(DecompIfstDesc), C.c_int, C.POINTER(_vp)]),
    'farnn_decomp_sf_max_create': (C.c_int, [C.POINTER(DecompIfstDesc), C.c_int, C.POINTER(_vp)]),
    'farnn_tag_vectors': (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    'farnn_tag_host_submit': (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    'farnn_flatten_host': (C.c_int64, [_vp, _vp, C.c_int32, C.c_int32, _vp]),
    'farnn_tag_host_wait': (C.c_int, [_vp, C.c_int32, _vp, C.POINTER(C.c_int64)]),
    'farnn_destroy': (None, [_vp]),
    'farnn_abi_version': (C.c_int, []),
    'farnn_ab_build': (C.c_int, []),
    'farnn_device_count': (C.c_int, []),
    'farnn_last_error': (C.c_char_p, []),
    'farnn_num_columns': (C.c_int, [_vp]),
    'farnn_algorithmic_bytes': (C.c_double, [_vp, C.c_int64]),
    'farnn_kernel_algorithmic_bytes': (C.c_double, [_vp, C.c_int32, C.c_int64]),
    'farnn_set_profiling': (C.c_int, [_vp, C.c_int32]),
    'farnn_kernel_time': (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'farnn_kernel_name': (C.c_char_p, [_vp, C.c_int32]),
}

_lib = None


def load():
    """Load libfarnn_hip.so (once).  Raises FarnnError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FarnnError(
            'HIP library not built: {} is missing. Run `python -c "import __graft_entry__ as g; '
            'g.build()"` (hipcc --offload-arch=gfx950). There is no CPU fallback.'.format(LIB_PATH))
    # PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  The tensors this
    # library receives live in THAT runtime's address space, so it must be the one already loaded
    # when libfarnn_hip.so resolves its HIP symbols: import torch first.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


AB_LIB_PATH = os.path.join(_HERE, 'csrc', 'libfarnn_hip_probes.so')     # the A/B (profiling) build: csrc/build.py --probes


def ab_build():
    """True when the loaded library is the A/B build (it carries the forms the production build left behind: FARNN_CV_ONE)."""
    return bool(load().farnn_ab_build())


def check(rc, what=''):
    if rc != OK:
        msg = load().farnn_last_error()
        raise FarnnError('{} failed with code {}: {}'.format(what or 'farnn call', rc,
                                                             msg.decode() if msg else ''))


def flatten_host(a_ptr, len_ptr, B, L, out_ptr):
    """utils.flatten of a host int64 [B,L] array into `out` (farnn_flatten_host); returns the element count."""
    return load().farnn_flatten_host(a_ptr, len_ptr, B, L, out_ptr)


def f32(a):
    """float32 C-contiguous numpy view/copy (the reference stores float64 and calls .float())."""
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def ptr(a):
    return None if a is None else a.ctypes.data_as(_f32p)


class Handle:
    """Owns one farnn_model*."""

    def __init__(self, raw, keepalive=()):
        self._raw = raw
        self._keep = keepalive

    @property
    def raw(self):
        if not self._raw:
            raise FarnnError('model handle already destroyed')
        return self._raw

    def close(self):
        if self._raw:
            load().farnn_destroy(self._raw)
            self._raw = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- thin wrappers -----------------------------------------------------------------------
    def num_columns(self):
        return load().farnn_num_columns(self.raw)

    def reserve(self, B, L):
        check(load().farnn_reserve(self.raw, B, L), 'farnn_reserve')

    def tag(self, x_ptr, len_ptr, B, L, mode, tags_ptr=None, flat_ptr=None, scores_ptr=None, stream=None):
        check(load().farnn_tag(self.raw, x_ptr, len_ptr, B, L, mode, tags_ptr, flat_ptr, scores_ptr,
                               stream), 'farnn_tag')

    def tag_vectors(self, v_ptr, len_ptr, B, L, mode=MODE_LOCAL, tags_ptr=None, flat_ptr=None, scores_ptr=None, stream=None):
        """farnn_tag on a vector-input handle (create_decomp_sf): v float32 [B, L, R] dense on the device, MODE_LOCAL only."""
        check(load().farnn_tag_vectors(self.raw, v_ptr, len_ptr, B, L, mode, tags_ptr, flat_ptr, scores_ptr,
                                       stream), 'farnn_tag_vectors')

    def tag_host_submit(self, x_ptr, len_ptr, B, L):
        """Host buffers in (int64 [B,L], [B]); returns a ticket for tag_host_wait.  Work is enqueued, not awaited."""
        t, n = C.c_int32(-1), C.c_int64(0)
        check(load().farnn_tag_host_submit(self.raw, x_ptr, len_ptr, B, L, C.byref(t), C.byref(n)), 'farnn_tag_host_submit')
        return t.value, n.value

    def tag_host_wait(self, ticket, flat_ptr):
        n = C.c_int64(0)
        check(load().farnn_tag_host_wait(self.raw, ticket, flat_ptr, C.byref(n)), 'farnn_tag_host_wait')
        return n.value

    def has_compact(self):
        return bool(load().farnn_has_compact(self.raw))

    def set_compact(self, enable=True):
        """Bit-packed blocks + active-state walk instead of the dense fp32 blocks (0/1 automata; include/farnn.h)."""
        check(load().farnn_set_compact(self.raw, int(bool(enable))), 'farnn_set_compact')

    def algorithmic_bytes(self, valid_tokens):
        return load().farnn_algorithmic_bytes(self.raw, int(valid_tokens))

    def kernel_algorithmic_bytes(self, which, valid_tokens):
        return load().farnn_kernel_algorithmic_bytes(self.raw, int(which), int(valid_tokens))

    def set_profiling(self, every):
        """every=0 off; every=N: time every N-th farnn_tag call with HIP events."""
        check(load().farnn_set_profiling(self.raw, int(every)), 'farnn_set_profiling')

    def kernel_time(self, which):
        ms, n = C.c_double(0), C.c_int64(0)
        check(load().farnn_kernel_time(self.raw, which, C.byref(ms), C.byref(n)), 'farnn_kernel_time')
        return ms.value, n.value

    def kernel_name(self, which):
        return load().farnn_kernel_name(self.raw, which).decode()


def _create(fn_name, desc, device, keep):
    lib = load()
    out = _vp()
    check(getattr(lib, fn_name)(C.byref(desc), int(device), C.byref(out)), fn_name)
    return Handle(out, keep)


def _dev_ptr(t):
    return C.cast(C.c_void_p(t.data_ptr()), _f32p)


def create_onehot_ifst(T, W, O, h0, hT, P=None, nl='none', semiring='sum', threshold=0.5, o_idx=0,
                       use_crf=False, crf_trans=None, device=0):
    """Weights as numpy arrays (host, copied by the library) or -- all of them -- as float32
    torch tensors already on the target device (weights_on_device=1; nothing crosses PCIe)."""
    import torch
    if torch.is_tensor(T):
        arrs = [a for a in (T, W, O, h0, hT, P, crf_trans) if a is not None]
        assert all(torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous()
                   for a in arrs), 'device weights must all be contiguous float32 CUDA tensors'
        V, S, _ = T.shape
        d = OnehotIfstDesc(V, S, O.shape[0], _dev_ptr(T), _dev_ptr(W), _dev_ptr(O), _dev_ptr(h0), _dev_ptr(hT),
                           None if P is None else _dev_ptr(P), NL[nl], SEMIRING[semiring], float(threshold),
                           int(o_idx), int(bool(use_crf)), None if crf_trans is None else _dev_ptr(crf_trans), 1)
        torch.cuda.synchronize(T.device)
        return _create('farnn_onehot_ifst_create', d, device, tuple(arrs))
    T, W, O, h0, hT = f32(T), f32(W), f32(O), f32(h0), f32(hT)
    P = None if P is None else f32(P)
    crf_trans = None if crf_trans is None else f32(crf_trans)
    V, S, _ = T.shape
    d = OnehotIfstDesc(V, S, O.shape[0], ptr(T), ptr(W), ptr(O), ptr(h0), ptr(hT), ptr(P),
                       NL[nl], SEMIRING[semiring], float(threshold), int(o_idx), int(bool(use_crf)),
                       ptr(crf_trans), 0)
    return _create('farnn_onehot_ifst_create', d, device, (T, W, O, h0, hT, P, crf_trans))


def _edge_list(word, frm, to, label, val):
    i32 = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.int32)      # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                     # noqa: E731
    word, frm, to, label = i32(word), i32(frm), i32(to), i32(label)
    n = word.shape[0]
    assert frm.shape == to.shape == label.shape == (n,)
    val = None if val is None else f32(val)
    return EdgeList(n, ip(word), ip(frm), ip(to), ip(label), ptr(val)), (word, frm, to, label, val)


def _create_from_edges(fn_name, base, edges, device, keep):
    lib = load()
    out = _vp()
    check(getattr(lib, fn_name)(C.byref(base), C.byref(edges), int(device), C.byref(out)), fn_name)
    return Handle(out, keep)


def create_onehot_ifst_from_edges(V, S, n_cols, word, frm, to, label, h0, hT, val=None, P=None, nl='none',
                                  semiring='sum', threshold=0.5, o_idx=0, use_crf=False, crf_trans=None,
                                  device=0):
    """The i-FST built on the device from the automaton's edge list (farnn_edge_list): no dense
    [V,S,S] tensor exists on the host.  `word` = -1 marks a wildcard edge, < -1 an entry that only
    labels its destination state; `label` < 0: no label."""
    edges, keep = _edge_list(word, frm, to, label, val)
    h0, hT = f32(h0), f32(hT)
    P = None if P is None else f32(P)
    crf_trans = None if crf_trans is None else f32(crf_trans)
    base = OnehotIfstDesc(int(V), int(S), int(n_cols), None, None, None, ptr(h0), ptr(hT), ptr(P),
                          NL[nl], SEMIRING[semiring], float(threshold), int(o_idx), int(bool(use_crf)),
                          ptr(crf_trans), 0)
    return _create_from_edges('farnn_onehot_ifst_create_from_edges', base, edges, device,
                              keep + (h0, hT, P, crf_trans))


def create_onehot_ifst_compact(V, S, n_cols, word, frm, to, label, h0, hT, val=None, P=None, nl='none', threshold=0.5,
                               o_idx=0, use_crf=False, crf_trans=None, device=0):
    """The i-FST in its compact form ONLY (bit-packed blocks scattered from the edge list; no dense tensor anywhere)."""
    edges, keep = _edge_list(word, frm, to, label, val)
    h0, hT = f32(h0), f32(hT)
    P = None if P is None else f32(P)
    crf_trans = None if crf_trans is None else f32(crf_trans)
    base = OnehotIfstDesc(int(V), int(S), int(n_cols), None, None, None, ptr(h0), ptr(hT), ptr(P),
                          NL[nl], SEMIRING['sum'], float(threshold), int(o_idx), int(bool(use_crf)),
                          ptr(crf_trans), 0)
    return _create_from_edges('farnn_onehot_ifst_create_compact', base, edges, device, keep + (h0, hT, P, crf_trans))


def create_onehot_fst4_from_edges(V, S, n_cols, word, frm, to, label, h0, hT, val=None, P=None, semiring='sum',
                                  threshold=0.5, o_idx=0, device=0):
    """FARNN_S_O (4-D FST) from the edge list: T4[w,l,f,t] / W4[l,f,t] are scattered on the device."""
    edges, keep = _edge_list(word, frm, to, label, val)
    h0, hT = f32(h0), f32(hT)
    P = None if P is None else f32(P)
    base = OnehotFst4Desc(int(V), int(S), int(n_cols), None, None, ptr(h0), ptr(hT), ptr(P),
                          SEMIRING[semiring], float(threshold), int(o_idx), 0)
    return _create_from_edges('farnn_onehot_fst4_create_from_edges', base, edges, device, keep + (h0, hT, P))


def create_onehot_ind1_from_edges(V, S, n_cols, word, frm, to, label, h0, hT, val=None, P=None, semiring='sum',
                                  mask_by_output=False, threshold=0.5, o_idx=0, device=0):
    """FARNN_S_O_I (independent=1) from the edge list: T, W and Oten[l,f,t] are scattered on the device."""
    edges, keep = _edge_list(word, frm, to, label, val)
    h0, hT = f32(h0), f32(hT)
    P = None if P is None else f32(P)
    base = OnehotInd1Desc(int(V), int(S), int(n_cols), None, None, None, ptr(h0), ptr(hT), ptr(P),
                          SEMIRING[semiring], int(bool(mask_by_output)), float(threshold), int(o_idx), 0)
    return _create_from_edges('farnn_onehot_ind1_create_from_edges', base, edges, device, keep + (h0, hT, P))


def create_onehot_fst4(T4, W4, h0, hT, P=None, semiring='sum', threshold=0.5, o_idx=0, device=0):
    T4, W4, h0, hT = f32(T4), f32(W4), f32(h0), f32(hT)
    P = None if P is None else f32(P)
    V, Cn, S, _ = T4.shape
    d = OnehotFst4Desc(V, S, Cn, ptr(T4), ptr(W4), ptr(h0), ptr(hT), ptr(P), SEMIRING[semiring],
                       float(threshold), int(o_idx), 0)
    return _create('farnn_onehot_fst4_create', d, device, (T4, W4, h0, hT, P))


def create_onehot_ind1(T, W, Oten, h0, hT, P=None, semiring='sum', mask_by_output=False, threshold=0.5,
                       o_idx=0, device=0):
    T, W, Oten, h0, hT = f32(T), f32(W), f32(Oten), f32(h0), f32(hT)
    P = None if P is None else f32(P)
    V, S, _ = T.shape
    d = OnehotInd1Desc(V, S, Oten.shape[0], ptr(T), ptr(W), ptr(Oten), ptr(h0), ptr(hT), ptr(P),
                       SEMIRING[semiring], int(bool(mask_by_output)), float(threshold), int(o_idx), 0)
    return _create('farnn_onehot_ind1_create', d, device, (T, W, Oten, h0, hT, P))


def create_decomp_ifst(Vgen, S1, S2, W, Cout, h0, hT, P=None, farnn=0, gates=None, sigmoid_exponent=5,
                       nl='none', semiring='sum', threshold=0.5, o_idx=0, use_crf=False, crf_trans=None,
                       device=0):
    Vgen, S1, S2, W, Cout, h0, hT = (f32(a) for a in (Vgen, S1, S2, W, Cout, h0, hT))
    P = None if P is None else f32(P)
    crf_trans = None if crf_trans is None else f32(crf_trans)
    g = {k: f32(v) for k, v in (gates or {}).items()}
    S, R = S1.shape
    d = DecompIfstDesc(Vgen.shape[0], S, R, Cout.shape[0], ptr(Vgen), ptr(S1), ptr(S2), ptr(W), ptr(Cout),
                       ptr(h0), ptr(hT), ptr(P), int(farnn),
                       ptr(g.get('Wss1')), ptr(g.get('Wrs1')), ptr(g.get('bs1')),
                       ptr(g.get('Wss2')), ptr(g.get('Wrs2')), ptr(g.get('bs2')),
                       float(sigmoid_exponent), NL[nl], SEMIRING[semiring], float(threshold), int(o_idx),
                       int(bool(use_crf)), ptr(crf_trans), 0)
    return _create('farnn_decomp_ifst_create', d, device, (Vgen, S1, S2, W, Cout, h0, hT, P, crf_trans, g))


def create_decomp_sf(S1, S2, W, Cout, h0, hT, P=None, farnn=0, gates=None, sigmoid_exponent=5, nl='none', semiring='sum',
                     threshold=0.5, o_idx=0, use_crf=False, crf_trans=None, device=0):
    """The decomposed i-FST on vectors (FARNN_S_SF): create_decomp_ifst without a word table; tag with Handle.tag_vectors."""
    S1, S2, W, Cout, h0, hT = (f32(a) for a in (S1, S2, W, Cout, h0, hT))
    P = None if P is None else f32(P)
    crf_trans = None if crf_trans is None else f32(crf_trans)
    g = {k: f32(v) for k, v in (gates or {}).items()}
    S, R = S1.shape
    d = DecompIfstDesc(0, S, R, Cout.shape[0], None, ptr(S1), ptr(S2), ptr(W), ptr(Cout),
                       ptr(h0), ptr(hT), ptr(P), int(farnn),
                       ptr(g.get('Wss1')), ptr(g.get('Wrs1')), ptr(g.get('bs1')),
                       ptr(g.get('Wss2')), ptr(g.get('Wrs2')), ptr(g.get('bs2')),
                       float(sigmoid_exponent), NL[nl], SEMIRING[semiring], float(threshold), int(o_idx),
                       int(bool(use_crf)), ptr(crf_trans), 0)
    return _create('farnn_decomp_sf_create', d, device, (S1, S2, W, Cout, h0, hT, P, crf_trans, g))


def create_decomp_sf_max(S1, S2, W, Cout, h0, hT, P=None, farnn=0, gates=None, sigmoid_exponent=5, nl='none', threshold=0.5,
                         o_idx=0, use_crf=False, crf_trans=None, device=0):
    """create_decomp_sf in the max semiring (farnn_decomp_sf_max_create): tagging only, with Handle.tag_vectors."""
    S1, S2, W, Cout, h0, hT = (f32(a) for a in (S1, S2, W, Cout, h0, hT))
    P = None if P is None else f32(P)
    crf_trans = None if crf_trans is None else f32(crf_trans)
    g = {k: f32(v) for k, v in (gates or {}).items()}
    S, R = S1.shape
    d = DecompIfstDesc(0, S, R, Cout.shape[0], None, ptr(S1), ptr(S2), ptr(W), ptr(Cout),
                       ptr(h0), ptr(hT), ptr(P), int(farnn),
                       ptr(g.get('Wss1')), ptr(g.get('Wrs1')), ptr(g.get('bs1')),
                       ptr(g.get('Wss2')), ptr(g.get('Wrs2')), ptr(g.get('bs2')),
                       float(sigmoid_exponent), NL[nl], SEMIRING['max'], float(threshold), int(o_idx),
                       int(bool(use_crf)), ptr(crf_trans), 0)
    return _create('farnn_decomp_sf_max_create', d, device, (S1, S2, W, Cout, h0, hT, P, crf_trans, g))


def create_decomp_ifst_folded(V_embed, E, G, beta, S1, S2, W, Cout, h0, hT, add_nl='none', normalize='none', P=None,
                              farnn=0, gates=None, sigmoid_exponent=5, nl='none', semiring='sum', threshold=0.5, o_idx=0,
                              use_crf=False, crf_trans=None, device=0):
    """create_decomp_ifst with the word table (and the per-rank --normalize_automata scaling of V_embed, S1, S2) computed on
    the device: Vgen = V_embed * beta + nl_add(E @ G) * (1 - beta).  G is the bridge of the UN-normalised V_embed."""
    V_embed, E, G, beta, S1, S2, W, Cout, h0, hT = (f32(a) for a in (V_embed, E, G, beta, S1, S2, W, Cout, h0, hT))
    P = None if P is None else f32(P)
    crf_trans = None if crf_trans is None else f32(crf_trans)
    g = {k: f32(v) for k, v in (gates or {}).items()}
    S, R = S1.shape
    d = DecompIfstDesc(V_embed.shape[0], S, R, Cout.shape[0], None, ptr(S1), ptr(S2), ptr(W), ptr(Cout),
                       ptr(h0), ptr(hT), ptr(P), int(farnn),
                       ptr(g.get('Wss1')), ptr(g.get('Wrs1')), ptr(g.get('bs1')),
                       ptr(g.get('Wss2')), ptr(g.get('Wrs2')), ptr(g.get('bs2')),
                       float(sigmoid_exponent), NL[nl], SEMIRING[semiring], float(threshold), int(o_idx),
                       int(bool(use_crf)), ptr(crf_trans), 0)
    fd = VgenFold(ptr(V_embed), ptr(E), ptr(G), ptr(beta), E.shape[1], NL[add_nl], NORM[normalize], 0)
    lib = load()
    out = _vp()
    check(lib.farnn_decomp_ifst_create_folded(C.byref(d), C.byref(fd), int(device), C.byref(out)),
          'farnn_decomp_ifst_create_folded')
    return Handle(out, (V_embed, E, G, beta, S1, S2, W, Cout, h0, hT, P, crf_trans, g))


def create_decomp_ind1(Vgen, S1, S2, W, Cout, S1o, S2o, h0, hT, Wo=None, P=None, farnn=0, gates=None,
                       sigmoid_exponent=5, nl='none', semiring='sum', threshold=0.5, o_idx=0, use_crf=False,
                       crf_trans=None, device=0):
    Vgen, S1, S2, W, Cout, S1o, S2o, h0, hT = (f32(a) for a in (Vgen, S1, S2, W, Cout, S1o, S2o, h0, hT))
    Wo = None if Wo is None else f32(Wo)
    P = None if P is None else f32(P)
    crf_trans = None if crf_trans is None else f32(crf_trans)
    g = {k: f32(v) for k, v in (gates or {}).items()}
    S, R = S1.shape
    K, RO = Cout.shape
    d = DecompInd1Desc(Vgen.shape[0], S, R, RO, K, ptr(Vgen), ptr(S1), ptr(S2), ptr(W), ptr(Cout),
                       ptr(S1o), ptr(S2o), ptr(Wo), ptr(h0), ptr(hT), ptr(P), int(farnn),
                       ptr(g.get('Wss1')), ptr(g.get('Wrs1')), ptr(g.get('bs1')),
                       ptr(g.get('Wss2')), ptr(g.get('Wrs2')), ptr(g.get('bs2')),
                       float(sigmoid_exponent), NL[nl], SEMIRING[semiring], float(threshold), int(o_idx),
                       int(bool(use_crf)), ptr(crf_trans), 0)
    return _create('farnn_decomp_ind1_create', d, device,
                   (Vgen, S1, S2, W, Cout, S1o, S2o, Wo, h0, hT, P, crf_trans, g))


def create_decomp_fst(Vgen, Cemb, S1, S2, Cw, S1w, S2w, WW, h0, hT, P=None, farnn=0, gates=None,
                      sigmoid_exponent=5, nl='none', semiring='sum', threshold=0.5, o_idx=0, use_crf=False,
                      crf_trans=None, device=0):
    Vgen, Cemb, S1, S2, Cw, S1w, S2w, WW, h0, hT = (
        f32(a) for a in (Vgen, Cemb, S1, S2, Cw, S1w, S2w, WW, h0, hT))
    P = None if P is None else f32(P)
    crf_trans = None if crf_trans is None else f32(crf_trans)
    g = {k: f32(v) for k, v in (gates or {}).items()}
    S, R = S1.shape
    K, RW = Cw.shape
    if Cemb.shape != (K, R):
        raise FarnnError('C_embed must be [K,R] = {}, got {}'.format((K, R), Cemb.shape))
    d = DecompFstDesc(Vgen.shape[0], S, R, RW, K, ptr(Vgen), ptr(Cemb), ptr(S1), ptr(S2), ptr(Cw),
                      ptr(S1w), ptr(S2w), ptr(WW), ptr(h0), ptr(hT), ptr(P), int(farnn),
                      ptr(g.get('Wss1')), ptr(g.get('Wrs1')), ptr(g.get('bs1')),
                      ptr(g.get('Wss2')), ptr(g.get('Wrs2')), ptr(g.get('bs2')),
                      float(sigmoid_exponent), NL[nl], SEMIRING[semiring], float(threshold), int(o_idx),
                      int(bool(use_crf)), ptr(crf_trans), 0)
    return _create('farnn_decomp_fst_create', d, device,
                   (Vgen, Cemb, S1, S2, Cw, S1w, S2w, WW, h0, hT, P, crf_trans, g))


class _TrainContextBase:
    """Owns one training context of the C-ABI (include/farnn.h).  A subclass names its five C symbols and its two struct types."""
    _create = _destroy = _step = _set_profiling = _time = None
    _weights = _outputs = None
    _set_semiring = None
    _raw = None

    def _open(self, dims, device, semiring='sum'):
        if semiring not in SEMIRING:             # before the native context exists: a bad name leaves no handle behind
            raise ValueError('semiring must be one of {}, not {!r}'.format(sorted(SEMIRING), semiring))
        out = C.c_void_p()
        check(getattr(load(), self._create)(C.byref(dims), int(device), C.byref(out)), self._create)
        self._raw = out
        self.semiring = 'sum'
        if semiring != 'sum':
            self.set_semiring(semiring)

    def set_semiring(self, semiring):
        """'sum' or 'max' (the reference's --train_mode) for the following steps."""
        check(getattr(load(), self._set_semiring)(self._raw, SEMIRING[semiring]), self._set_semiring)
        self.semiring = semiring

    def close(self):
        if self._raw:
            getattr(load(), self._destroy)(self._raw)
            self._raw = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, weights, x_ptr, len_ptr, labels_ptr, B, L, valid_tokens, outputs, stream=None):
        """weights / outputs: dicts of device pointers (ints) keyed like the C structs."""
        w = self._weights(**{k: (weights.get(k) or None) for k, _ in self._weights._fields_})
        o = self._outputs(**{k: outputs.get(k) for k, _ in self._outputs._fields_})
        check(getattr(load(), self._step)(self._raw, C.byref(w), x_ptr, len_ptr, labels_ptr, int(B), int(L),
                                          int(valid_tokens), C.byref(o), stream), self._step)

    def set_profiling(self, enable):
        check(getattr(load(), self._set_profiling)(self._raw, int(enable)), self._set_profiling)

    def time(self):
        ms, n = C.c_double(0), C.c_int64(0)
        check(getattr(load(), self._time)(self._raw, C.byref(ms), C.byref(n)), self._time)
        return ms.value, n.value


class TrainContext(_TrainContextBase):
    """Owns one farnn_train_ctx* (training step of the decomposed i-FST, include/farnn.h)."""
    _create, _destroy, _step = 'farnn_train_create', 'farnn_train_destroy', 'farnn_decomp_ifst_train_step'
    _set_profiling, _time = 'farnn_train_set_profiling', 'farnn_train_time'
    _set_semiring = 'farnn_train_set_semiring'
    _weights, _outputs = TrainWeights, TrainOutputs

    def __init__(self, V, S, R, K, nl='none', threshold=0.5, o_idx=0, device=0, use_crf=False, farnn=0,
                 sigmoid_exponent=5.0, semiring='sum', teacher_max=False):
        self._open(TrainDims(int(V), int(S), int(R), int(K), NL[nl], float(threshold), int(o_idx), int(farnn),
                             float(sigmoid_exponent), int(bool(use_crf))), device, semiring)
        self.dims = (int(V), int(S), int(R), int(K))
        # the KD / PR teacher in the max semiring is opt-in for its first release: without it teacher_step() on a max context
        # goes to the sum entry as before, and that entry refuses the context
        self.teacher_max = bool(teacher_max)

    def teacher_step(self, weights, x_ptr, len_ptr, labels_ptr, re_ptr, mode, c1, pi, B, L, valid_tokens, outputs, stream=None,
                     max_entry=None):
        """step() with the KD / PR teacher: re_ptr is the device pointer of the float [B][L][K] teacher scores, mode 'kd' or
        'pr' (or the raw FARNN_TEACHER_* value), pi the weight of the original loss.  The entry is the context's semiring's:
        farnn_decomp_ifst_teacher_train_step (sum) or, on a context opened with teacher_max=True,
        farnn_decomp_ifst_teacher_max_train_step (max).  max_entry = True / False names the entry instead (each refuses a
        context in the other semiring)."""
        w = self._weights(**{k: (weights.get(k) or None) for k, _ in self._weights._fields_})
        o = self._outputs(**{k: outputs.get(k) for k, _ in self._outputs._fields_})
        t = Teacher(int(TEACHER.get(mode, mode)), float(c1), float(pi))
        if max_entry is None:
            max_entry = self.semiring == 'max' and self.teacher_max
        entry = 'farnn_decomp_ifst_teacher_max_train_step' if max_entry else 'farnn_decomp_ifst_teacher_train_step'
        check(getattr(load(), entry)(self._raw, C.byref(w), x_ptr, len_ptr, labels_ptr, re_ptr, C.byref(t),
                                     int(B), int(L), int(valid_tokens), C.byref(o), stream), entry)


class SfTrainContext(TrainContext):
    """Owns one farnn_train_ctx* made by farnn_decomp_sf_train_create: the training step of the vector-input i-FST (FARNN_S_SF;
    include/farnn.h).  Sum semiring only, no teacher: set_semiring('max'), step() and teacher_step() are refused
    by the library on such a context."""
    _create = 'farnn_decomp_sf_train_create'

    def __init__(self, S, R, K, nl='none', threshold=0.5, o_idx=0, device=0, use_crf=False, farnn=0, sigmoid_exponent=5.0):
        super().__init__(0, S, R, K, nl=nl, threshold=threshold, o_idx=o_idx, device=device, use_crf=use_crf, farnn=farnn,
                         sigmoid_exponent=sigmoid_exponent)

    def step_vectors(self, weights, v_ptr, len_ptr, labels_ptr, B, L, valid_tokens, outputs, dv_ptr, stream=None):
        """farnn_decomp_sf_train_step: v_ptr / dv_ptr are the device pointers of the float [B][L][R] input and its gradient;
        weights / outputs as step()'s, without Vgen / dVgen."""
        w = self._weights(**{k: (weights.get(k) or None) for k, _ in self._weights._fields_})
        o = self._outputs(**{k: outputs.get(k) for k, _ in self._outputs._fields_})
        check(load().farnn_decomp_sf_train_step(self._raw, C.byref(w), v_ptr, len_ptr, labels_ptr, int(B), int(L),
                                                int(valid_tokens), C.byref(o), dv_ptr, stream), 'farnn_decomp_sf_train_step')


class DecompFstTrainContext(_TrainContextBase):
    """Owns one farnn_decomp_fst_train_ctx* (training step of the decomposed FST, FARNN_S_D_W; include/farnn.h)."""
    _create, _destroy, _step = 'farnn_decomp_fst_train_create', 'farnn_decomp_fst_train_destroy', 'farnn_decomp_fst_train_step'
    _set_profiling, _time = 'farnn_decomp_fst_train_set_profiling', 'farnn_decomp_fst_train_time'
    _set_semiring = 'farnn_decomp_fst_train_set_semiring'
    _weights, _outputs = DecompFstTrainWeights, DecompFstTrainOutputs

    def __init__(self, V, S, R, Q, K, nl='none', threshold=0.5, o_idx=0, device=0, use_crf=False, farnn=0, sigmoid_exponent=5.0,
                 semiring='sum'):
        self._open(DecompFstTrainDims(int(V), int(S), int(R), int(Q), int(K), NL[nl], float(threshold), int(o_idx), int(farnn),
                                      float(sigmoid_exponent), int(bool(use_crf))), device, semiring)
        self.dims = (int(V), int(S), int(R), int(Q), int(K))


class OnehotTrainContext(_TrainContextBase):
    """Owns one farnn_onehot_train_ctx* (training step of the onehot i-FST, include/farnn.h)."""
    _create, _destroy, _step = 'farnn_onehot_train_create', 'farnn_onehot_train_destroy', 'farnn_onehot_ifst_train_step'
    _set_profiling, _time = 'farnn_onehot_train_set_profiling', 'farnn_onehot_train_time'
    _set_semiring = 'farnn_onehot_train_set_semiring'
    _weights, _outputs = OnehotTrainWeights, OnehotTrainOutputs

    def __init__(self, V, S, n_cols, nl='none', threshold=0.5, o_idx=0, device=0, semiring='sum'):
        self._open(OnehotTrainDims(int(V), int(S), int(n_cols), NL[nl], float(threshold), int(o_idx)), device, semiring)
        self.dims = (int(V), int(S), int(n_cols))


class Fst4TrainContext(_TrainContextBase):
    """Owns one farnn_fst4_train_ctx* (training step of the onehot FST, include/farnn.h)."""
    _create, _destroy, _step = 'farnn_fst4_train_create', 'farnn_fst4_train_destroy', 'farnn_fst4_train_step'
    _set_profiling, _time = 'farnn_fst4_train_set_profiling', 'farnn_fst4_train_time'
    _set_semiring = 'farnn_fst4_train_set_semiring'
    _weights, _outputs = Fst4TrainWeights, Fst4TrainOutputs

    def __init__(self, V, S, n_cols, threshold=0.5, o_idx=0, device=0, semiring='sum'):
        self._open(Fst4TrainDims(int(V), int(S), int(n_cols), float(threshold), int(o_idx)), device, semiring)
        self.dims = (int(V), int(S), int(n_cols))


class Ind1TrainContext(_TrainContextBase):
    """Owns one farnn_ind1_train_ctx* (training step of the onehot independent=1 model, include/farnn.h)."""
    _create, _destroy, _step = 'farnn_ind1_train_create', 'farnn_ind1_train_destroy', 'farnn_ind1_train_step'
    _set_profiling, _time = 'farnn_ind1_train_set_profiling', 'farnn_ind1_train_time'
    _set_semiring = 'farnn_ind1_train_set_semiring'
    _weights, _outputs = Ind1TrainWeights, Ind1TrainOutputs

    def __init__(self, V, S, n_cols, mask_by_output=False, threshold=0.5, o_idx=0, device=0, semiring='sum'):
        self._open(Ind1TrainDims(int(V), int(S), int(n_cols), int(bool(mask_by_output)), float(threshold), int(o_idx)),
                   device, semiring)
        self.dims = (int(V), int(S), int(n_cols))


class Decomp1TrainContext(_TrainContextBase):
    """Owns one farnn_decomp_ind1_train_ctx* (training step of the decomposed independent=1 model, include/farnn.h)."""
    _create, _destroy = 'farnn_decomp_ind1_train_create', 'farnn_decomp_ind1_train_destroy'
    _step = 'farnn_decomp_ind1_train_step'
    _set_profiling, _time = 'farnn_decomp_ind1_train_set_profiling', 'farnn_decomp_ind1_train_time'
    _set_semiring = 'farnn_decomp_ind1_train_set_semiring'
    _weights, _outputs = Decomp1TrainWeights, Decomp1TrainOutputs

    def __init__(self, V, S, R, RO, n_cols, nl='none', threshold=0.5, o_idx=0, device=0, semiring='sum'):
        self._open(Decomp1TrainDims(int(V), int(S), int(R), int(RO), int(n_cols), NL[nl], float(threshold), int(o_idx)), device,
                   semiring)
        self.dims = (int(V), int(S), int(R), int(RO), int(n_cols))

    def step_crf(self, weights, trans_ptr, x_ptr, len_ptr, labels_ptr, B, L, valid_tokens, outputs, dtrans_ptr, stream=None):
        """step() under --use_crf 1 (farnn_decomp_ind1_crf_train_step): trans_ptr / dtrans_ptr are the device pointers of the
        float [C][C] CRF transitions and of their gradient; n_cols counts START and STOP."""
        w = self._weights(**{k: (weights.get(k) or None) for k, _ in self._weights._fields_})
        o = self._outputs(**{k: outputs.get(k) for k, _ in self._outputs._fields_})
        check(load().farnn_decomp_ind1_crf_train_step(self._raw, C.byref(w), trans_ptr, x_ptr, len_ptr, labels_ptr, int(B), int(L),
                                                      int(valid_tokens), C.byref(o), dtrans_ptr, stream),
              'farnn_decomp_ind1_crf_train_step')

    def gated_step(self, weights, farnn, sigmoid_exponent, x_ptr, len_ptr, labels_ptr, B, L, valid_tokens, outputs, stream=None,
                   trans_ptr=None, dtrans_ptr=None, entry='farnn_decomp_ind1_gated_train_step'):
        """step() for the gated model (farnn_decomp_ind1_gated_train_step): `weights` holds Wss1 .. bs2 beside the plain step's
        weights and `outputs` dWss1 .. dbs2 beside its outputs (farnn = 1: the second gate's stay None); trans_ptr / dtrans_ptr
        as step_crf's, both None for the CE1 loss."""
        w = self._weights(**{k: (weights.get(k) or None) for k, _ in self._weights._fields_})
        o = self._outputs(**{k: outputs.get(k) for k, _ in self._outputs._fields_})
        g = Decomp1GateWeights(int(farnn), *[(weights.get(k) or None) for k in ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')],
                               float(sigmoid_exponent))
        go = Decomp1GateOutputs(*[outputs.get(k) for k in ('dWss1', 'dWrs1', 'dbs1', 'dWss2', 'dWrs2', 'dbs2')])
        check(getattr(load(), entry)(self._raw, C.byref(w), C.byref(g), trans_ptr, x_ptr, len_ptr, labels_ptr, int(B), int(L),
                                     int(valid_tokens), C.byref(o), C.byref(go), dtrans_ptr, stream), entry)

    def gated_max_step(self, *args, **kwargs):
        """gated_step() on a max context (farnn_decomp_ind1_gated_max_train_step): the same arguments."""
        self.gated_step(*args, entry='farnn_decomp_ind1_gated_max_train_step', **kwargs)


class Optim:
    """Owns one farnn_optim* (the multi-tensor optimizer step, include/farnn.h): the chunk table of the tensors' sizes and
    their step counts.  Parameters, gradients and moments stay the caller's; step() takes their device pointers."""

    def __init__(self, kind, numel, lr, beta1=0.9, beta2=0.999, eps=1e-8, device=0):
        self._raw = None
        self.n = len(numel)
        self.lr = float(lr)
        sizes = (C.c_int64 * max(self.n, 1))(*[int(v) for v in numel])
        out = C.c_void_p()
        check(load().farnn_optim_create(C.byref(OptimDesc(int(kind), self.lr, float(beta1), float(beta2), float(eps))), sizes,
                                        self.n, int(device), C.byref(out)), 'farnn_optim_create')
        self._raw = out
        self._arrays = tuple((C.c_void_p * self.n)() for _ in range(4))      # params, grads, exp_avg, exp_avg_sq

    def close(self):
        if self._raw:
            load().farnn_optim_destroy(self._raw)
            self._raw = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, params, grads, exp_avg=None, exp_avg_sq=None, stream=None):
        """params / grads / exp_avg / exp_avg_sq: sequences of device pointers (ints; None or 0 in grads: that tensor is
        skipped).  exp_avg and exp_avg_sq are None for SGD."""
        P, G, M, V = self._arrays
        for i in range(self.n):
            P[i], G[i] = params[i], grads[i]
            if exp_avg is not None:
                M[i], V[i] = exp_avg[i], exp_avg_sq[i]
        check(load().farnn_optim_step(self._raw, P, G, None if exp_avg is None else M, None if exp_avg is None else V, stream),
              'farnn_optim_step')

    def set_lr(self, lr):
        check(load().farnn_optim_set_lr(self._raw, float(lr)), 'farnn_optim_set_lr')
        self.lr = float(lr)

    def steps(self, i):
        n = C.c_int64(0)
        check(load().farnn_optim_steps(self._raw, int(i), C.byref(n)), 'farnn_optim_steps')
        return n.value

    def set_steps(self, i, n):
        check(load().farnn_optim_set_steps(self._raw, int(i), int(n)), 'farnn_optim_set_steps')


class Score:
    """Owns one farnn_score* (the device-side scorer, include/farnn.h): the label tables, the counts and what one add leaves
    for the next.  add() takes device pointers and waits for nothing; read() is the only call that waits."""

    def __init__(self, kind, type_, canon, n_types, o_idx, device=0):
        self._raw = None
        self.n_labels, self.n_types = len(kind), int(n_types)
        arrays = [None if a is None else (C.c_int32 * max(len(a), 1))(*[int(v) for v in a]) for a in (kind, type_, canon)]
        out = C.c_void_p()
        check(load().farnn_score_create(C.byref(out), arrays[0], arrays[1], arrays[2], self.n_labels, self.n_types, int(o_idx),
                                        int(device)), 'farnn_score_create')
        self._raw = out
        self._per_type = (C.c_int64 * max(SCORE_TYPE_ROWS * self.n_types, 1))()

    def close(self):
        if self._raw:
            load().farnn_score_destroy(self._raw)
            self._raw = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, tags_ptr, labels_ptr, len_ptr, B, L, loss_ptr=None, stream=None):
        check(load().farnn_score_add(self._raw, tags_ptr, labels_ptr, len_ptr, int(B), int(L), loss_ptr, stream), 'farnn_score_add')

    def read(self, stream=None):
        """(ScoreCounts, [SCORE_TYPE_ROWS][n_types] lists)"""
        c = ScoreCounts()
        c.per_type = C.cast(self._per_type, C.POINTER(C.c_int64))
        check(load().farnn_score_read(self._raw, C.byref(c), stream), 'farnn_score_read')
        nt = self.n_types
        return c, [[int(self._per_type[r * nt + t]) for t in range(nt)] for r in range(SCORE_TYPE_ROWS)]

    def reset(self, stream=None):
        check(load().farnn_score_reset(self._raw, stream), 'farnn_score_reset')


ENUMERIC, ERANGE, EINVAL = -33, -34, -22       # FARNN_ENUMERIC, FARNN_ERANGE, FARNN_EINVAL
CP_CHUNK, CP_PANEL, CP_TILE, CP_MAX_RANK = 64, 1024, 16, 352      # csrc/cp_als.hip.h


class CpContext:
    """Owns one farnn_cp_ctx* (float64 CP-ALS of a 3-way or 4-way tensor given as a coordinate list, include/farnn.h).  A failed
    call raises FarnnError with the return code in `.code`, except FARNN_ENUMERIC (a singular normal matrix), which raises
    numpy.linalg.LinAlgError like the solve of the library it stands in for.

    ``CpContext(dims, idx0, idx1, idx2, val, max_rank)`` is the 3-way form on the 3-way entries; ``CpContext.from_coo(dims,
    idx_list, val, max_rank)`` takes 3 or 4 index arrays and goes through the farnn_cp_*_n entries."""

    def __init__(self, dims, idx0, idx1, idx2, val, max_rank, device=0):
        self._raw = None
        self._n = False
        i32 = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.int32)      # noqa: E731
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                     # noqa: E731
        idx0, idx1, idx2 = i32(idx0), i32(idx1), i32(idx2)
        val = np.ascontiguousarray(np.asarray(val), dtype=np.float64)
        n = val.shape[0]
        if not (idx0.shape == idx1.shape == idx2.shape == val.shape == (n,)):
            raise ValueError('idx0, idx1, idx2 and val must be one-dimensional and equally long')
        self.dims = tuple(int(d) for d in dims)
        d = (C.c_int32 * 3)(*self.dims)
        out = C.c_void_p()
        self._check(load().farnn_cp_create(d, n, ip(idx0), ip(idx1), ip(idx2), val.ctypes.data_as(C.POINTER(C.c_double)),
                                           int(max_rank), int(device), C.byref(out)), 'farnn_cp_create')
        self._raw = out
        self.max_rank = int(max_rank)

    @classmethod
    def from_coo(cls, dims, idx_list, val, max_rank, device=0):
        """A tensor of order len(dims) = len(idx_list), 3 or 4, through farnn_cp_create_n (which refuses every other order)."""
        self = cls.__new__(cls)
        self._raw = None
        self._n = True
        idx = [np.ascontiguousarray(np.asarray(a), dtype=np.int32) for a in idx_list]
        val = np.ascontiguousarray(np.asarray(val), dtype=np.float64)
        n = val.shape[0] if val.ndim == 1 else -1
        if len(idx) != len(dims) or any(a.shape != (n,) for a in idx):
            raise ValueError('one index array per dimension, each one-dimensional and as long as val')
        self.dims = tuple(int(d) for d in dims)
        d = (C.c_int32 * max(len(self.dims), 1))(*self.dims)
        ip = (C.c_void_p * max(len(idx), 1))(*[a.ctypes.data for a in idx])
        out = C.c_void_p()
        self._check(load().farnn_cp_create_n(len(self.dims), d, n, ip, val.ctypes.data_as(C.POINTER(C.c_double)), int(max_rank),
                                             int(device), C.byref(out)), 'farnn_cp_create_n')
        self._raw = out
        self.max_rank = int(max_rank)
        return self

    @property
    def order(self):
        n = C.c_int32(0)
        self._check(load().farnn_cp_order(self._raw, C.byref(n)), 'farnn_cp_order')
        return n.value

    @staticmethod
    def _ptr_array(ptrs):
        return (C.c_void_p * len(ptrs))(*[None if p is None else int(p) for p in ptrs])

    @staticmethod
    def _check(rc, what):
        if rc == OK:
            return
        msg = load().farnn_last_error()
        text = '{} failed with code {}: {}'.format(what, rc, msg.decode() if msg else '')
        if rc == ENUMERIC:
            raise np.linalg.LinAlgError(text)
        err = FarnnError(text)
        err.code = rc
        raise err

    def close(self):
        if self._raw:
            load().farnn_cp_destroy(self._raw)
            self._raw = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def norm2(self):
        """(||X||^2, distinct coordinates)"""
        v, n = C.c_double(0), C.c_int64(0)
        self._check(load().farnn_cp_norm2(self._raw, C.byref(v), C.byref(n)), 'farnn_cp_norm2')
        return v.value, n.value

    def mttkrp(self, mode, rank, f_ptrs, out_ptr, stream=None):
        """f_ptrs: the factors' device pointers, one per mode (the one of `mode` may be None)"""
        if len(f_ptrs) != len(self.dims):
            raise ValueError('one factor pointer per mode')
        if self._n:
            self._check(load().farnn_cp_mttkrp_n(self._raw, int(mode), int(rank), self._ptr_array(f_ptrs), out_ptr, stream),
                        'farnn_cp_mttkrp_n')
            return
        self._check(load().farnn_cp_mttkrp(self._raw, int(mode), int(rank), f_ptrs[0], f_ptrs[1], f_ptrs[2], out_ptr, stream),
                    'farnn_cp_mttkrp')

    def normal_matrix(self, mode, rank, f_ptrs, H_ptr, stream=None):
        if len(f_ptrs) != len(self.dims):
            raise ValueError('one factor pointer per mode')
        if self._n:
            self._check(load().farnn_cp_normal_matrix_n(self._raw, int(mode), int(rank), self._ptr_array(f_ptrs), H_ptr, stream),
                        'farnn_cp_normal_matrix_n')
            return
        self._check(load().farnn_cp_normal_matrix(self._raw, int(mode), int(rank), f_ptrs[0], f_ptrs[1], f_ptrs[2], H_ptr, stream),
                    'farnn_cp_normal_matrix')

    def solve(self, rank, H_ptr, M_ptr, rows, out_ptr, stream=None):
        self._check(load().farnn_cp_solve(self._raw, int(rank), H_ptr, M_ptr, int(rows), out_ptr, stream), 'farnn_cp_solve')

    def run(self, rank, n_iter_max, tol, factors, stream=None):
        """factors: one float64 array [dim_n, rank] per mode (the initial factors; not modified).  Returns (factors, rec_errors)."""
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                    # noqa: E731
        f = [np.array(a, dtype=np.float64, order='C') for a in factors]
        if len(f) != len(self.dims):
            raise ValueError('one factor per mode')
        for a, d in zip(f, self.dims):
            if a.shape != (d, int(rank)):
                raise ValueError('a factor must be [dim, rank] = {}, got {}'.format((d, int(rank)), a.shape))
        errs = np.zeros(max(int(n_iter_max), 1), dtype=np.float64)
        n = C.c_int32(0)
        if self._n:
            self._check(load().farnn_cp_run_n(self._raw, int(rank), int(n_iter_max), float(tol),
                                              self._ptr_array([a.ctypes.data for a in f]), dp(errs), C.byref(n), stream),
                        'farnn_cp_run_n')
            return f, [float(e) for e in errs[:n.value]]
        self._check(load().farnn_cp_run(self._raw, int(rank), int(n_iter_max), float(tol), dp(f[0]), dp(f[1]), dp(f[2]), dp(errs),
                                        C.byref(n), stream), 'farnn_cp_run')
        return f, [float(e) for e in errs[:n.value]]

    def set_profiling(self, enable):
        self._check(load().farnn_cp_set_profiling(self._raw, int(bool(enable))), 'farnn_cp_set_profiling')

    def time(self):
        """({'normal_matrix', 'mttkrp', 'solve', 'error'}: milliseconds summed, timed sweeps)"""
        ms, n = (C.c_double * 4)(), C.c_int64(0)
        self._check(load().farnn_cp_time(self._raw, ms, C.byref(n)), 'farnn_cp_time')
        return dict(zip(('normal_matrix', 'mttkrp', 'solve', 'error'), [float(v) for v in ms])), n.value
