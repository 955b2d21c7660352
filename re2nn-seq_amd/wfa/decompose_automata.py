"""Automaton -> decomposed-model pickles: the reference's ``src_seq/wfa/decompose_automata.py`` on the library's CP-ALS
(wfa/tensor_func.py).  Same names, rank tables, seed arithmetic (``rands = rands + k * 8``), best-of-``k_best`` by the last
error, pickle schema (init_params.py documents it) and file names; the data directory, the output directory and the rank lists
are optional arguments with the reference's values as defaults.

    python -m re2nn_seq_amd.wfa.decompose_automata --dataset D --automata_path P --independent 0|1|2
           [--ranks 100,150] [--output_ranks 70] [--wildcard_ranks 70] [--k_best K] [--data_dir DIR] [--out_dir DIR]

``--independent 0`` (``decompose_automata``, the ``D.automata`` writer) decomposes the 4-way tensor; its
pickle is keyed by the outer seeds 0 .. 3, not by the reference's mutated loop variable (see its docstring)."""
import argparse
import os
import pickle
from copy import copy, deepcopy

from numpy.linalg import LinAlgError

from . import tensor_func
from ..data import load_slot_dataset
from ..utils import create_datetime_str, load_pkl
from .fsa_to_tensor import dfa_to_edges_slot_new, dfa_to_tensor_slot_independent_wildcard, dfa_to_tensor_slot_single_wildcard

DATA_DIR = '../../data/'
OUTPUT_TENSOR_RANKS = [70, 100, 150]
WILDCARD_TENSOR_RANKS = [70, 100, 150]      # ref :60
N_SEEDS = 4


def ranks_single(dataset_name):
    """ref :341-358"""
    return {'MITR': [100, 150, 200], 'MITR-BIO': [250, 300], 'MITM-E-BIO': [200, 250, 300], 'ATIS-BIO': [100, 150, 200],
            'ATIS-ZH-BIO': [300], 'SNIPS-BIO': [200, 250, 300], 'CONLL03-BIO': [100, 150, 200]}.get(dataset_name, [100, 150, 200])


def ranks_independent(dataset_name):
    """ref :174-187"""
    return {'MITR': [100, 150, 200], 'MITR-BIO': [150, 200, 250], 'MITM-E-BIO': [150, 200, 250], 'ATIS-BIO': [100, 150, 200],
            'ATIS-ZH-BIO': [150, 200, 250], 'CONLL03-BIO': [100, 150, 200]}.get(dataset_name, [100, 150, 200])


def _best_of(k_best, rands, decompose, make_dict, copier, catch):
    """The reference's restart loop: `rands` grows by k * 8 before every try, a try that raises `catch` is skipped, the lowest
    last error wins.  Returns (best dict or None, lowest error, rands)."""
    lowest_rec_error = float('inf')
    best_save_dict = None
    for k in range(k_best):
        print('BEST of {}: {}'.format(k_best, k))
        rands = rands + k * 8
        try:
            result = decompose(rands)
        except catch:
            print('Value Error or LinAlgError')
            continue
        rec_error = result[-1]
        if rec_error[-1] < lowest_rec_error:
            best_save_dict = copier(make_dict(*result[:-1]))
            lowest_rec_error = rec_error[-1]
    return best_save_dict, lowest_rec_error, rands


def _dump(obj, out_dir, kind, dataset_name, time_str, init, k_best, n_states, automata_name, split_group, info_str, rule_name):
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, '{kind}.automata.{time_str}.{init}.{k}best.{n}states.{automata_name}.{split}splits.{info}.'
                                 '{rule_name}.pkl'.format(kind=kind, time_str=time_str, init=init, k=k_best, n=n_states,
                                                          automata_name=automata_name, split=split_group, info=info_str,
                                                          rule_name=rule_name))
    with open(path, 'wb') as f:
        pickle.dump(obj, f)
    print('FINISHED')
    return path


def _out_dir(out_dir, data_dir, dataset_name):
    return out_dir if out_dir is not None else os.path.join(data_dir, dataset_name, 'automata')


def ranks_fst(dataset_name):
    """ref :41-54"""
    return {'MITR': [100, 150, 200], 'MITR-BIO': [150, 200, 250], 'MITM-E-BIO': [150, 200, 250], 'ATIS-BIO': [100, 150, 200],
            'ATIS-ZH-BIO': [150, 200, 250], 'CONLL03-BIO': [100, 150, 200]}.get(dataset_name, [100, 150, 200])


def decompose_automata(rearranged_automata, dataset_name, automata_name, split_group, init='random', k_best=5, rule_name='',
                       data_dir=DATA_DIR, out_dir=None, ranks=None, wildcard_tensor_ranks=None):
    """ref :17-145: D.automata.*.pkl (--independent 0), the 4-way language tensor [V', C, S, S] and the 3-way wildcard tensor
    [C, S, S].  Returns the path written.  The 4-way tensor goes to the library as coordinates (dfa_to_edges_slot_new); its dense
    form is never built.

    One deliberate difference.  The reference's restart line ``random_state = random_state + k * 8`` changes the outer loop's own
    variable, so its pickle is keyed by the value that variable has reached (480 .. 483 at the defaults), which the loader's
    ``automata_dicts[args.seed]`` cannot find for seeds 0 .. 3.  Here the ARITHMETIC of the draws is the reference's -- the running
    value starts at the outer seed, grows by k * 8 before every try, is carried from the wildcard ranks into the ranks and is not
    reset within an outer seed -- but the pickle is keyed by the outer seeds 0 .. 3, like the other two writers' and like
    synth.make_d_pickle_dict.

    An automaton without a single edge is refused before anything is read: its tensors have no nonzero, and the CP-ALS takes no
    tensor whose norm is zero (farnn_cp_create_n: FARNN_EINVAL)."""
    if not any(labels for fanout in (rearranged_automata.get('transitions') or {}).values() for labels in fanout.values()):
        raise NotImplementedError('decomposing an automaton without edges is not built: its tensors have no nonzero, which the '
                                  'CP-ALS refuses (DESIGN.md row f13)')
    print('AUTOMATA TO TENSOR')
    print('Total States: {}'.format(len(rearranged_automata['states'])))
    data = load_slot_dataset(dataset_name, data_dir)
    word2idx, slot2idx = data['t2i'], data['s2i']
    word, label, frm, to, dims, state2idx, wildcard_tensor, wildcard_wildcard_tensor, final_vector, start_vector, language = \
        dfa_to_edges_slot_new(rearranged_automata, word2idx, slot2idx, dataset=dataset_name)

    print('DECOMPOSE SPLIT AUTOMATA')
    ranks = ranks_fst(dataset_name) if ranks is None else list(ranks)
    wildcard_tensor_ranks = WILDCARD_TENSOR_RANKS if wildcard_tensor_ranks is None else list(wildcard_tensor_ranks)
    time_str = create_datetime_str()
    n_states = len(rearranged_automata['states'])
    all_decomposed_automata = dict()
    all_decomposed_automata['automata'] = rearranged_automata
    print(language)
    info_str = ''
    for random_state in range(N_SEEDS):
        rands = random_state
        wildcard_factor_dicts = dict()
        for wildcard_tensor_rank in wildcard_tensor_ranks:
            print('DECOMPOSING WILDCARD TENSOR RANK: {}, TENSOR SIZE: {}'.format(wildcard_tensor_rank, wildcard_tensor.shape))
            best, _, rands = _best_of(
                k_best, rands,
                lambda r: tensor_func.decompose_tensor_split_slot_3d(wildcard_tensor, wildcard_tensor_rank, random_state=r,
                                                                     init='random', verbose=1, n_iter_max=10),
                lambda C, S1, S2: {'C_wildcard': C, 'S1_wildcard': S1, 'S2_wildcard': S2},
                copy, ValueError)
            wildcard_factor_dicts[wildcard_tensor_rank] = best

        info_str = ''
        factor_dicts = dict()
        for rank in ranks:
            print('DECOMPOSING RANK: {}, NON-NEGATIV: {}, TENSOR SIZE: {}'.format(rank, False, dims))
            best, lowest, rands = _best_of(
                k_best, rands,
                lambda r: tensor_func.decompose_tensor_split_slot_4d_edges(word, label, frm, to, dims, language, word2idx, rank,
                                                                           random_state=r, init=init, verbose=1, n_iter_max=10),
                lambda V, C, S1, S2: {'V': V, 'C': C, 'S1': S1, 'S2': S2, 'wildcard_tensor': wildcard_tensor,
                                      'wildcard_wildcard_tensor': wildcard_wildcard_tensor},
                deepcopy, (ValueError, LinAlgError))
            factor_dicts[rank] = best
            info_str += '{}:{},'.format(rank, lowest.__round__(4))
        all_decomposed_automata[random_state] = [factor_dicts, wildcard_factor_dicts]

    return _dump(all_decomposed_automata, _out_dir(out_dir, data_dir, dataset_name), 'D', dataset_name, time_str, init, k_best,
                 n_states, automata_name, split_group, info_str, rule_name)


def decompose_automata_independent(rearranged_automata, dataset_name, automata_name, split_group, init='random', k_best=5,
                                   rule_name='', data_dir=DATA_DIR, out_dir=None, ranks=None, output_tensor_ranks=None):
    """ref :148-312: IID.automata.*.pkl (--independent 1).  Returns the path written."""
    print('AUTOMATA TO TENSOR')
    print('Total States: {}'.format(len(rearranged_automata['states'])))
    data = load_slot_dataset(dataset_name, data_dir)
    word2idx, slot2idx = data['t2i'], data['s2i']
    # (the reference's dfa_to_tensor_slot_independent is the _wildcard layout with the `oo` slice split off)
    language_tensor, state2idx, wildcard_mat, new_output_tensor, _, final_vector, start_vector, language = \
        dfa_to_tensor_slot_independent_wildcard(rearranged_automata, word2idx, slot2idx, dataset=dataset_name)
    output_tensor, output_wildcard_mat = new_output_tensor[:-1], new_output_tensor[-1]

    print('DECOMPOSE SPLIT AUTOMATA')
    ranks = ranks_independent(dataset_name) if ranks is None else list(ranks)
    output_tensor_ranks = OUTPUT_TENSOR_RANKS if output_tensor_ranks is None else list(output_tensor_ranks)
    time_str = create_datetime_str()
    n_states = len(rearranged_automata['states'])
    all_decomposed_automata = dict()
    all_decomposed_automata['automata'] = rearranged_automata
    info_str = ''
    for random_state in range(N_SEEDS):
        rands = random_state
        output_factor_dicts = dict()       # C related params
        output_factor_dicts_w = dict()     # C+1 related params
        for output_tensor_rank in output_tensor_ranks:
            print('DECOMPOSING WILDCARD TENSOR RANK: {}, TENSOR SIZE: {}'.format(output_tensor_rank, output_tensor.shape))
            best, _, rands = _best_of(
                k_best, rands,
                lambda r: tensor_func.decompose_tensor_split_slot_3d(output_tensor, output_tensor_rank, random_state=r, init=init,
                                                                     verbose=1, n_iter_max=40),
                lambda C, S1, S2: {'C_output': C, 'S1_output': S1, 'S2_output': S2, 'wildcard_output': output_wildcard_mat},
                copy, ValueError)
            output_factor_dicts[output_tensor_rank] = best
            print('DECOMPOSING NEW WILDCARD TENSOR RANK: {}, TENSOR SIZE: {}'.format(output_tensor_rank, new_output_tensor.shape))
            best, _, rands = _best_of(
                k_best, rands,
                lambda r: tensor_func.decompose_tensor_split_slot_3d(new_output_tensor, output_tensor_rank, random_state=r,
                                                                     init=init, verbose=1, n_iter_max=40),
                lambda C, S1, S2: {'C_output': C, 'S1_output': S1, 'S2_output': S2, 'wildcard_output': None},
                deepcopy, ValueError)
            output_factor_dicts_w[output_tensor_rank] = best

        info_str = ''
        factor_dicts = dict()
        rands = 0
        for rank in ranks:
            print('DECOMPOSING RANK: {}, TENSOR SIZE: {}'.format(rank, language_tensor.shape))
            best, lowest, rands = _best_of(
                k_best, rands,
                lambda r: tensor_func.decompose_tensor_split_slot_3d_language(language_tensor, language=language, word2idx=word2idx,
                                                                              rank=rank, random_state=r, n_iter_max=40, init=init,
                                                                              verbose=1),
                lambda V, S1, S2: {'V': V, 'S1': S1, 'S2': S2, 'wildcard_mat': wildcard_mat},
                copy, (ValueError, LinAlgError))
            factor_dicts[rank] = best
            info_str += '{}-{}'.format(rank, lowest.__round__(4))
        all_decomposed_automata[random_state] = [factor_dicts, output_factor_dicts, output_factor_dicts_w]

    return _dump(all_decomposed_automata, _out_dir(out_dir, data_dir, dataset_name), 'IID', dataset_name, time_str, init, k_best,
                 n_states, automata_name, split_group, info_str, rule_name)


def decompose_automata_single(rearranged_automata, dataset_name, automata_name, split_group, init='random', k_best=2, rule_name='',
                              data_dir=DATA_DIR, out_dir=None, ranks=None):
    """ref :315-433: IIID.automata.*.pkl (--independent 2).  Returns the path written."""
    print('AUTOMATA TO TENSOR')
    print('Total States: {}'.format(len(rearranged_automata['states'])))
    data = load_slot_dataset(dataset_name, data_dir)
    word2idx, slot2idx = data['t2i'], data['s2i']
    # (the reference's dfa_to_tensor_slot_single is the _wildcard layout with the `oo` row split off)
    language_tensor, state2idx, wildcard_mat, output_mat_new, _, final_vector, start_vector, language = \
        dfa_to_tensor_slot_single_wildcard(rearranged_automata, word2idx, slot2idx, dataset=dataset_name)
    output_mat, output_wildcard_vector = output_mat_new[:-1], output_mat_new[-1]

    print('DECOMPOSE SPLIT AUTOMATA')
    ranks = ranks_single(dataset_name) if ranks is None else list(ranks)
    time_str = create_datetime_str()
    n_states = len(rearranged_automata['states'])
    output_factor_dicts = {'output_mat': output_mat, 'output_wildcard_vector': output_wildcard_vector}
    output_factor_dicts_w = {'output_mat': output_mat_new, 'output_wildcard_vector': output_wildcard_vector}
    all_decomposed_automata = dict()
    all_decomposed_automata['automata'] = rearranged_automata
    print(language)
    info_str = ''
    for random_state in range(N_SEEDS):
        info_str = ''
        factor_dicts = dict()
        rands = random_state
        for rank in ranks:
            print('DECOMPOSING RANK: {}, TENSOR SIZE: {}'.format(rank, language_tensor.shape))
            best, lowest, rands = _best_of(
                k_best, rands,
                lambda r: tensor_func.decompose_tensor_split_slot_3d_language(language_tensor, language=language, word2idx=word2idx,
                                                                              rank=rank, random_state=r, n_iter_max=32, init=init,
                                                                              verbose=1),
                lambda V, S1, S2: {'V': V, 'S1': S1, 'S2': S2, 'wildcard_mat': wildcard_mat},
                copy, (ValueError, LinAlgError))
            factor_dicts[rank] = best
            info_str += '{}-{}'.format(rank, lowest.__round__(4))
        all_decomposed_automata[random_state] = [factor_dicts, output_factor_dicts, output_factor_dicts_w]

    return _dump(all_decomposed_automata, _out_dir(out_dir, data_dir, dataset_name), 'IIID', dataset_name, time_str, init, k_best,
                 n_states, automata_name, split_group, info_str, rule_name)


def _int_list(text):
    return [int(v) for v in text.split(',') if v]


def main(argv=None):
    p = argparse.ArgumentParser(description='decompose an automaton into the pickles --method decompose loads')
    p.add_argument('--dataset', required=True)
    p.add_argument('--automata_path', required=True, help='the automaton pickle (the dict itself or {"automata": dict})')
    p.add_argument('--independent', type=int, required=True, choices=[0, 1, 2])
    p.add_argument('--ranks', type=_int_list, default=None)
    p.add_argument('--output_ranks', type=_int_list, default=None)
    p.add_argument('--wildcard_ranks', type=_int_list, default=None)
    p.add_argument('--k_best', type=int, default=None)
    p.add_argument('--data_dir', default=DATA_DIR)
    p.add_argument('--out_dir', default=None)
    p.add_argument('--automata_name', default=None)
    p.add_argument('--split_group', type=int, default=1)
    p.add_argument('--rule_name', default='')
    args = p.parse_args(argv)
    automata = load_pkl(args.automata_path)
    if 'automata' in automata:
        automata = automata['automata']
    name = args.automata_name or os.path.basename(args.automata_path)
    if args.independent == 0:
        return decompose_automata(automata, args.dataset, name, args.split_group, k_best=args.k_best or 5, rule_name=args.rule_name,
                                  data_dir=args.data_dir, out_dir=args.out_dir, ranks=args.ranks,
                                  wildcard_tensor_ranks=args.wildcard_ranks)
    if args.independent == 1:
        return decompose_automata_independent(automata, args.dataset, name, args.split_group, k_best=args.k_best or 5,
                                              rule_name=args.rule_name, data_dir=args.data_dir, out_dir=args.out_dir,
                                              ranks=args.ranks, output_tensor_ranks=args.output_ranks)
    return decompose_automata_single(automata, args.dataset, name, args.split_group, k_best=args.k_best or 2,
                                     rule_name=args.rule_name, data_dir=args.data_dir, out_dir=args.out_dir, ranks=args.ranks)


if __name__ == '__main__':
    print(main())
