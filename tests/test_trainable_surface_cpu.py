"""The training surface the five trainable mirrors share (farnn/_trainable.py), without a GPU: every refusal's type and text,
that a model without its opt-in is refused before its args are read, the names / order / flags of the parameters
enable_training() builds (Adam state and farnn.optim are positional) with the semiring its context is opened in, and that
a switch counts only at the value '1'.  The literal strings and lists are those of the five hand-made copies this surface
replaced."""
import pytest
import torch

import trainable_models as tm

NO_STEP = ('training epochs are implemented for the i-FST models only (--independent 2: --method decompose, DESIGN.md row f3, '
           'and --method onehot, row f5); {} has no training step, run it with --epoch 0')
IFST_MODE = ('training the onehot i-FST covers the sum semiring only by default; --train_mode max is opt-in (set '
             'RE2NN_ONEHOT_MAX_TRAIN=1), --train_mode {} was asked for (DESIGN.md, row f5)')
FST_MODE = 'training the onehot FST covers the sum semiring only, --train_mode {} was asked for (DESIGN.md, row f7)'
IND1_MODE = 'training the onehot independent=1 model covers the sum semiring only, --train_mode {} was asked for (DESIGN.md, row f8)'
D1 = ('training the decomposed independent=1 model covers farnn 0, the sum semiring and the CE1 loss on one GPU; {} is not built '
      '(DESIGN.md, row f9)')
D_IFST = ('the HIP training step covers the sum and max semirings and the CE1 loss (with or without the CRF), no KD/PR teachers '
          '(DESIGN.md, row f3)')
D_IFST_MAX = ('the KD / PR teacher terms are built for the sum semiring only; --train_mode max walks the valid positions only '
              '(DESIGN.md, row f3)')

# (kind, args fields, switches set to '1', ranks, exception, message); every model's own opt-in is set unless the row is about it
REFUSALS = [
    ('onehot_ifst', dict(train_mode='max'), (), 1, NotImplementedError, IFST_MODE.format('max')),
    ('onehot_ifst', dict(train_mode='both'), ('RE2NN_ONEHOT_MAX_TRAIN',), 1, NotImplementedError, IFST_MODE.format('both')),
    ('onehot_ifst', dict(local_loss_func='CE'), (), 1, NotImplementedError,
     'training the onehot i-FST covers the CE1 loss only (main.py:127)'),
    ('onehot_ifst', dict(crf=True), (), 1, NotImplementedError,
     "training the onehot i-FST with the CRF extension (enable_crf) is not built; the reference's onehot models never read "
     'use_crf (DESIGN.md, row f5)'),
    ('onehot_ifst', {}, (), 2, NotImplementedError,
     'multi-GPU data-parallel training of the onehot i-FST is not built; train on one GPU (DESIGN.md, row f5)'),
    ('onehot_fst', dict(no_opt_in=True), (), 1, NotImplementedError, NO_STEP.format('FARNN_S_O')),
    ('onehot_fst', dict(train_mode='max'), (), 1, NotImplementedError, FST_MODE.format('max')),
    ('onehot_fst', dict(train_mode='both'), ('RE2NN_BUCKETED_MAX_TRAIN',), 1, NotImplementedError, FST_MODE.format('both')),
    ('onehot_fst', dict(local_loss_func='CE'), (), 1, NotImplementedError,
     'training the onehot FST covers the CE1 loss only (main.py:127)'),
    ('onehot_fst', dict(train_wildcard_wildcard=1), (), 1, NotImplementedError,
     'training the onehot FST with --train_wildcard_wildcard 1 is not built: wildcard_wildcard_mat is not read under CE1 and '
     'has no gradient (DESIGN.md, row f7)'),
    ('onehot_fst', {}, (), 2, NotImplementedError,
     'multi-GPU data-parallel training of the onehot FST is not built; train on one GPU (DESIGN.md, row f7)'),
    ('onehot_ind1', dict(no_opt_in=True), (), 1, NotImplementedError, NO_STEP.format('FARNN_S_O_I')),
    ('onehot_ind1', dict(train_mode='max'), (), 1, NotImplementedError, IND1_MODE.format('max')),
    ('onehot_ind1', dict(train_mode='both'), ('RE2NN_BUCKETED_MAX_TRAIN',), 1, NotImplementedError, IND1_MODE.format('both')),
    ('onehot_ind1', dict(local_loss_func='CE'), (), 1, NotImplementedError,
     'training the onehot independent=1 model covers the CE1 loss only (main.py:127)'),
    ('onehot_ind1', {}, (), 2, NotImplementedError,
     'multi-GPU data-parallel training of the onehot independent=1 model is not built; train on one GPU (DESIGN.md, row f8)'),
    ('decomp_ind1', dict(no_opt_in=True), (), 1, NotImplementedError, NO_STEP.format('FARNN_S_D_W_I')),
    ('decomp_ind1', dict(farnn=1), (), 1, NotImplementedError, D1.format('the gated recurrences (--farnn 1)')),
    ('decomp_ind1', dict(farnn=2), (), 1, NotImplementedError, D1.format('the gated recurrences (--farnn 2)')),
    ('decomp_ind1', dict(train_mode='max'), (), 1, NotImplementedError, D1.format('the max semiring (--train_mode max)')),
    ('decomp_ind1', dict(train_mode='both'), ('RE2NN_BUCKETED_MAX_TRAIN',), 1, NotImplementedError,
     D1.format('the max semiring (--train_mode both)')),
    ('decomp_ind1', dict(use_crf=1), (), 1, NotImplementedError, D1.format('the CRF (--use_crf 1)')),
    ('decomp_ind1', dict(local_loss_func='CE'), (), 1, NotImplementedError, D1.format('a loss other than CE1 (--local_loss_func CE)')),
    ('decomp_ind1', dict(marryup_type='kd'), (), 1, NotImplementedError, D1.format('the KD / PR teacher terms (--marryup_type kd)')),
    ('decomp_ind1', dict(marryup_type='pr'), ('RE2NN_DECOMP_TEACHER_TRAIN',), 1, NotImplementedError,
     D1.format('the KD / PR teacher terms (--marryup_type pr)')),
    ('decomp_ind1', {}, (), 2, NotImplementedError, D1.format('multi-GPU data-parallel training')),
    ('decomp_ifst', dict(train_mode='both'), (), 1, NotImplementedError, D_IFST),
    ('decomp_ifst', dict(local_loss_func='CE'), (), 1, NotImplementedError, D_IFST),
    ('decomp_ifst', dict(farnn=3), (), 1, NotImplementedError, D_IFST),
    ('decomp_ifst', dict(marryup_type='kd', re=True), (), 1, NotImplementedError, D_IFST),
    ('decomp_ifst', dict(marryup_type='pr', re=True), ('RE2NN_DECOMP_TEACHER_MAX_TRAIN',), 1, NotImplementedError, D_IFST),
    ('decomp_ifst', dict(marryup_type='input'), ('RE2NN_DECOMP_TEACHER_TRAIN',), 1, NotImplementedError, D_IFST),
    ('decomp_ifst', dict(marryup_type='kd', train_mode='max', re=True), ('RE2NN_DECOMP_TEACHER_TRAIN',), 1, NotImplementedError,
     D_IFST_MAX),
    ('decomp_ifst', dict(marryup_type='kd'), ('RE2NN_DECOMP_TEACHER_TRAIN',), 1, ValueError,
     "--marryup_type kd needs the RE teacher's scores: forward_local(..., re_tags=...)"),
    ('decomp_ifst', dict(re=True), ('RE2NN_DECOMP_TEACHER_TRAIN',), 1, ValueError,
     "re_tags were given but --marryup_type is 'none': the teacher term would be dropped silently"),
]


def _environment(monkeypatch, kind, on=(), own=True):
    for name in tm.ALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name in on + ((tm.SWITCH[kind],) if own and kind in tm.SWITCH else ()):
        monkeypatch.setenv(name, '1')


def _no_device(monkeypatch):
    """from here on no GPU is visible and any use of the HIP library fails the test"""
    from re2nn_seq_amd import _lib

    def boom(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for name in ('OnehotTrainContext', 'Fst4TrainContext', 'Ind1TrainContext', 'TrainContext', 'Decomp1TrainContext', 'load'):
        monkeypatch.setattr(_lib, name, boom)


def _batch(with_re):
    x = torch.zeros((2, 3), dtype=torch.int64)
    return x, x, torch.tensor([3, 2]), torch.zeros((2, 3, tm.C)) if with_re else None


@pytest.mark.parametrize('kind,kw,on,ranks,exc,text', REFUSALS, ids=lambda v: None)
def test_every_refusal_keeps_its_type_and_text(monkeypatch, kind, kw, on, ranks, exc, text):
    from re2nn_seq_amd import dist
    from re2nn_seq_amd.train_onehot import check_trainable
    kw = dict(kw)
    own, crf, with_re = not kw.pop('no_opt_in', False), kw.pop('crf', False), kw.pop('re', False)
    _environment(monkeypatch, kind, on, own)
    m = tm.build(kind, **kw)
    if crf:
        m.enable_crf()
    _no_device(monkeypatch)
    monkeypatch.setattr(dist, 'world', lambda: (0, ranks))
    x, lab, lengths, re = _batch(with_re)
    calls = [lambda: m.forward_local(x, lab, lengths, train=True, re_tags=re)]
    if kind == 'decomp_ifst':                              # its check needs the batch's re_tags: forward_local alone runs it
        calls.append(lambda: m._check_trainable(re))
    else:
        calls += [m.enable_training, lambda: check_trainable(m), m._check_trainable]
    for call in calls:
        with pytest.raises(exc) as e:
            call()
        assert type(e.value) is exc and str(e.value) == text


def test_the_decomposed_ifst_is_checked_in_forward_local_only(monkeypatch):
    """enable_training() and train_onehot.check_trainable() do not run its check (it needs re_tags): an uncovered configuration
    gets as far as the missing device, or passes"""
    from re2nn_seq_amd import _lib
    from re2nn_seq_amd.train_onehot import check_trainable
    _environment(monkeypatch, 'decomp_ifst')
    m = tm.build('decomp_ifst', local_loss_func='CE')
    _no_device(monkeypatch)
    check_trainable(m)
    with pytest.raises(_lib.FarnnError, match='no MI355X visible; the training step has no CPU fallback'):
        m.enable_training()


@pytest.mark.parametrize('kind', ['onehot_fst', 'onehot_ind1', 'decomp_ind1'])
def test_without_its_opt_in_a_model_is_refused_before_its_args_are_read(monkeypatch, kind):
    from re2nn_seq_amd.train_onehot import check_trainable
    _environment(monkeypatch, kind, own=False)
    cls = tm.cls_of(kind)
    m = cls.__new__(cls)                                   # no args, no attribute at all
    _no_device(monkeypatch)
    x, lab, lengths, _ = _batch(False)
    for call in (m._check_trainable, m.enable_training, lambda: check_trainable(m),
                 lambda: m.forward_local(x, lab, lengths, train=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == NO_STEP.format(cls.__name__)


D_IFST_ALL = ['S1', 'S2', 'embed_r_generalized', 'V_embed', 'C_output_mat', 'wildcard_mat', 'h0', 'hT', 'beta_vec', 'embedding.weight']
D_IND1_ALL = ['S1', 'S2', 'embed_r_generalized', 'V_embed', 'C_output', 'S1_output', 'S2_output', 'wildcard_mat', 'h0', 'hT',
              'beta_vec', 'embedding.weight']
GATES1, GATES2 = ['Wss1', 'Wrs1', 'bs1'], ['Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2']
ALL_ON = dict(train_wildcard=1, train_wildcard_wildcard=1, train_h0=1, train_hT=1, train_beta=1, train_V_embed=1, train_word_embed=1)
CRF_ON = ('RE2NN_DECOMP_IND1_CRF_TRAIN',)

# (kind, args fields, switches, every tensor of _tp in order, the ones named_parameters() yields in order)
PARAMETERS = [
    ('onehot_ifst', {}, (), ['language_tensor', 'wildcard_mat', 'output_mat', 'h0', 'hT'], ['language_tensor']),
    ('onehot_ifst', ALL_ON, (), ['language_tensor', 'wildcard_mat', 'output_mat', 'h0', 'hT'], ['language_tensor']),
    ('onehot_fst', {}, (), ['language_tensor', 'wildcard_tensor', 'h0', 'hT'], ['language_tensor']),
    ('onehot_fst', dict(train_wildcard=1, train_h0=1, train_hT=1), (), ['language_tensor', 'wildcard_tensor', 'h0', 'hT'],
     ['language_tensor', 'wildcard_tensor']),
    ('onehot_ind1', {}, (), ['language_tensor', 'wildcard_mat', 'output_tensor', 'h0', 'hT'], ['language_tensor']),
    ('onehot_ind1', ALL_ON, (), ['language_tensor', 'wildcard_mat', 'output_tensor', 'h0', 'hT'], ['language_tensor']),
    ('decomp_ifst', {}, (), D_IFST_ALL, ['S1', 'S2', 'embed_r_generalized', 'C_output_mat']),
    ('decomp_ifst', dict(train_c_output=0), (), D_IFST_ALL, ['S1', 'S2', 'embed_r_generalized']),
    ('decomp_ifst', dict(train_wildcard=1), (), D_IFST_ALL, ['S1', 'S2', 'embed_r_generalized', 'C_output_mat', 'wildcard_mat']),
    ('decomp_ifst', dict(train_h0=1), (), D_IFST_ALL, ['S1', 'S2', 'embed_r_generalized', 'C_output_mat', 'h0']),
    ('decomp_ifst', dict(train_hT=1), (), D_IFST_ALL, ['S1', 'S2', 'embed_r_generalized', 'C_output_mat', 'hT']),
    ('decomp_ifst', dict(train_beta=1), (), D_IFST_ALL, ['S1', 'S2', 'embed_r_generalized', 'C_output_mat', 'beta_vec']),
    ('decomp_ifst', dict(train_V_embed=1), (), D_IFST_ALL, ['S1', 'S2', 'embed_r_generalized', 'V_embed', 'C_output_mat']),
    ('decomp_ifst', dict(train_word_embed=1), (), D_IFST_ALL, ['S1', 'S2', 'embed_r_generalized', 'C_output_mat', 'embedding.weight']),
    ('decomp_ifst', ALL_ON, (), D_IFST_ALL, D_IFST_ALL),
    ('decomp_ifst', dict(farnn=1), (), D_IFST_ALL + GATES1, ['S1', 'S2', 'embed_r_generalized', 'C_output_mat'] + GATES1),
    ('decomp_ifst', dict(farnn=2), (), D_IFST_ALL + GATES2, ['S1', 'S2', 'embed_r_generalized', 'C_output_mat'] + GATES2),
    ('decomp_ifst', dict(use_crf=1), (), D_IFST_ALL + ['crf.transitions'],
     ['S1', 'S2', 'embed_r_generalized', 'C_output_mat', 'crf.transitions']),
    ('decomp_ifst', dict(ALL_ON, farnn=2, use_crf=1), (), D_IFST_ALL + GATES2 + ['crf.transitions'],
     D_IFST_ALL + GATES2 + ['crf.transitions']),
    ('decomp_ind1', {}, (), D_IND1_ALL, ['S1', 'S2', 'embed_r_generalized']),
    ('decomp_ind1', dict(train_wildcard=1), (), D_IND1_ALL, ['S1', 'S2', 'embed_r_generalized', 'C_output', 'S1_output', 'S2_output']),
    ('decomp_ind1', dict(train_wildcard_wildcard=1), (), D_IND1_ALL, ['S1', 'S2', 'embed_r_generalized', 'wildcard_mat']),
    ('decomp_ind1', dict(train_h0=1), (), D_IND1_ALL, ['S1', 'S2', 'embed_r_generalized', 'h0']),
    ('decomp_ind1', dict(train_hT=1), (), D_IND1_ALL, ['S1', 'S2', 'embed_r_generalized', 'hT']),
    ('decomp_ind1', dict(train_beta=1), (), D_IND1_ALL, ['S1', 'S2', 'embed_r_generalized', 'beta_vec']),
    ('decomp_ind1', dict(train_V_embed=1), (), D_IND1_ALL, ['S1', 'S2', 'embed_r_generalized', 'V_embed']),
    ('decomp_ind1', dict(train_word_embed=1), (), D_IND1_ALL, ['S1', 'S2', 'embed_r_generalized', 'embedding.weight']),
    ('decomp_ind1', dict(use_crf=1), CRF_ON, D_IND1_ALL + ['crf.transitions'], ['S1', 'S2', 'embed_r_generalized', 'crf.transitions']),
    ('decomp_ind1', dict(ALL_ON, use_crf=1), CRF_ON, D_IND1_ALL + ['crf.transitions'], D_IND1_ALL + ['crf.transitions']),
]
CONTEXT = {'onehot_ifst': 'OnehotTrainContext', 'onehot_fst': 'Fst4TrainContext', 'onehot_ind1': 'Ind1TrainContext',
           'decomp_ifst': 'TrainContext', 'decomp_ind1': 'Decomp1TrainContext'}
MAX_SWITCH = {'onehot_ifst': 'RE2NN_ONEHOT_MAX_TRAIN', 'onehot_fst': 'RE2NN_BUCKETED_MAX_TRAIN', 'onehot_ind1': 'RE2NN_BUCKETED_MAX_TRAIN',
              'decomp_ifst': None, 'decomp_ind1': 'RE2NN_BUCKETED_MAX_TRAIN'}


def _host_device(monkeypatch):
    """enable_training() without a GPU: the device is the host and every context constructor records its arguments"""
    from re2nn_seq_amd import _lib
    from re2nn_seq_amd.farnn._native import NativeTagger
    opened = []
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(NativeTagger, '_dev', lambda self: torch.device('cpu'))
    for name in set(CONTEXT.values()):
        monkeypatch.setattr(_lib, name, lambda *a, _name=name, **k: opened.append((_name, a, k)) or object())
    return opened


@pytest.mark.parametrize('mode', ['sum', 'max'])
@pytest.mark.parametrize('kind,kw,on,every,trained', PARAMETERS, ids=lambda v: None)
def test_parameter_names_order_and_flags(monkeypatch, kind, kw, on, every, trained, mode):
    _environment(monkeypatch, kind, on + ((MAX_SWITCH[kind],) if mode == 'max' and MAX_SWITCH[kind] else ()))
    m = tm.build(kind, train_mode=mode, **kw)               # before the patch: the constructor asks for the current device
    opened = _host_device(monkeypatch)
    assert list(m.parameters()) == [] and list(m.named_parameters()) == []
    assert m.enable_training() is m
    assert list(m._tp) == every
    named = list(m.named_parameters())
    assert [k for k, _ in named] == trained
    assert all(t.requires_grad and t.is_leaf and t.dtype == torch.float32 for _, t in named)
    assert all(a is b for (_, a), b in zip(named, m.parameters())) and len(list(m.parameters())) == len(named)
    assert all(m._tp[k] is t for k, t in named)
    assert not any(m._tp[k].requires_grad for k in every if k not in trained)
    assert m._tpP is None and m._dirty is False
    assert [(name, k['semiring']) for name, _, k in opened] == [(CONTEXT[kind], mode)]
    assert m.enable_training() is m and len(opened) == 1      # the second call builds nothing


def test_the_priority_matrix_goes_to_the_device_only_with_use_priority(monkeypatch):
    _environment(monkeypatch, 'onehot_ifst')
    m = tm.build('onehot_ifst', use_priority=1)
    _host_device(monkeypatch)
    m.enable_training()
    assert m._tpP.dtype == torch.float32 and tuple(m._tpP.shape) == m.priority_full.shape


def _opens(kind, check_args=(), **kw):
    def probe():
        try:
            tm.build(kind, **kw)._check_trainable(*check_args)
        except NotImplementedError:
            return False
        return True
    return probe


RE = (torch.zeros((2, 3, tm.C)),)
# (switch, the other switches it stands beside, what it opens)
SWITCHES = [
    ('RE2NN_ONEHOT_MAX_TRAIN', (), _opens('onehot_ifst', train_mode='max')),
    ('RE2NN_ONEHOT_FST_TRAIN', (), _opens('onehot_fst')),
    ('RE2NN_ONEHOT_IND1_TRAIN', (), _opens('onehot_ind1')),
    ('RE2NN_DECOMP_IND1_TRAIN', (), _opens('decomp_ind1')),
    ('RE2NN_DECOMP_IND1_CRF_TRAIN', ('RE2NN_DECOMP_IND1_TRAIN',), _opens('decomp_ind1', use_crf=1)),
    ('RE2NN_BUCKETED_MAX_TRAIN', ('RE2NN_ONEHOT_FST_TRAIN',), _opens('onehot_fst', train_mode='max')),
    ('RE2NN_BUCKETED_MAX_TRAIN', ('RE2NN_ONEHOT_IND1_TRAIN',), _opens('onehot_ind1', train_mode='max')),
    ('RE2NN_BUCKETED_MAX_TRAIN', ('RE2NN_DECOMP_IND1_TRAIN',), _opens('decomp_ind1', train_mode='max')),
    ('RE2NN_DECOMP_TEACHER_TRAIN', (), _opens('decomp_ifst', RE, marryup_type='kd')),
    ('RE2NN_DECOMP_TEACHER_MAX_TRAIN', ('RE2NN_DECOMP_TEACHER_TRAIN',), _opens('decomp_ifst', RE, marryup_type='pr', train_mode='max')),
]


@pytest.mark.parametrize('switch,beside,opens', SWITCHES, ids=lambda v: v if isinstance(v, str) else None)
def test_a_switch_counts_only_at_the_value_1(monkeypatch, switch, beside, opens):
    from re2nn_seq_amd.farnn._native import opted_in
    for name in tm.ALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name in beside:
        monkeypatch.setenv(name, '1')
    _no_device(monkeypatch)
    assert not opens() and not opted_in(switch[len('RE2NN_'):])
    for value in ('0', 'true', '', '11', ' 1'):
        monkeypatch.setenv(switch, value)
        assert not opens() and not opted_in(switch[len('RE2NN_'):]), value
    monkeypatch.setenv(switch, '1')
    assert opens() and opted_in(switch[len('RE2NN_'):])


@pytest.mark.parametrize('value,want', [(None, False), ('0', False), ('true', False), ('1', True)])
def test_the_teacher_max_switch_reaches_the_context_and_the_optimizer_switch_its_reader(monkeypatch, value, want):
    from re2nn_seq_amd.farnn._native import bucketed_max_train_enabled, opted_in
    _environment(monkeypatch, 'decomp_ifst')
    for name in ('RE2NN_DECOMP_TEACHER_MAX_TRAIN', 'RE2NN_NATIVE_OPTIM', 'RE2NN_BUCKETED_MAX_TRAIN'):
        if value is not None:
            monkeypatch.setenv(name, value)
    m = tm.build('decomp_ifst')
    opened = _host_device(monkeypatch)
    m.enable_training()
    assert opened[0][2]['teacher_max'] is want
    assert opted_in('NATIVE_OPTIM') is want and bucketed_max_train_enabled() is want
