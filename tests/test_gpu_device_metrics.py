"""The device-side scorer on the GPU (farnn_score_*, metrics/device.py): every count of read() against the
numpy restatement over the concatenated flat lists and the final tuples against metrics.py -- exact equality -- on streams with
planted boundary cases, on random dense streams, at the edges of the kernel's constants (64 positions per pass, SCORE_WAVES
sequences in flight, 64 sequences per resolving pass), with ids outside the tables, across reset, with the loss sum, through
the command line with the switch off and on, and through val_onehot."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

I2S = {0: 'o', 1: 'B-a', 2: 'I-a', 3: 'B-b', 4: 'i-b', 5: 'B-c', 6: 'I-c', 7: 'B-a', 8: '<pad>'}
O, Ba, Ia, Bb, Ib, Bc, Ic, Ba2, PAD = range(9)
STRAY = 1000                 # what the padding holds: outside the tables, so reading it would show in `errors`


def _tables():
    from re2nn_seq_amd.metrics import device as D
    return D.label_tables(I2S, O)


def _batch(seqs, L, B=None):
    """[(pred list, gold list)] -> tags int32 [B, L], labels int64 [B, L], lengths int64 [B]; the padding holds STRAY"""
    B = len(seqs) if B is None else B
    tags, labels, lengths = np.full((B, L), STRAY, np.int32), np.full((B, L), STRAY, np.int64), np.zeros(B, np.int64)
    for b, (p, g) in enumerate(seqs):
        assert len(p) == len(g) <= L
        tags[b, :len(p)], labels[b, :len(g)], lengths[b] = p, g, len(p)
    return tags, labels, lengths


def _flat(batches):
    pred = [t[b, :n] for t, _, ln in batches for b, n in enumerate(ln)]
    gold = [g[b, :n] for _, g, ln in batches for b, n in enumerate(ln)]
    return np.concatenate(pred).astype(np.int64), np.concatenate(gold).astype(np.int64)


def _score():
    from re2nn_seq_amd.metrics.device import DeviceScore
    return DeviceScore(I2S, O, 0)


def _run(score, batches, losses=None):
    dev = torch.device('cuda', 0)
    for i, (t, g, ln) in enumerate(batches):
        score.add(torch.from_numpy(t).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(ln).to(dev),
                  loss=None if losses is None else losses[i])
    return score.read()


def _assert_all_equal(got, batches):
    """every count against the restatement on the concatenated lists, the tuples against metrics.py"""
    from re2nn_seq_amd.metrics import device as D
    from re2nn_seq_amd.metrics.metrics import eval_seq_token, get_ner_fmeasure
    pred, gold = _flat(batches)
    want = D.counts_from_flat(pred, gold, _tables())
    assert got.integers() == want.integers()
    assert got.adds == len(batches)
    if want.errors == 0 and want.n > 0:
        assert D.token_level(got) == eval_seq_token(pred, gold, o_idx=O)
        ent, ref = D.entity_level(got, all_class=True), get_ner_fmeasure(gold, pred, i2s=I2S, all_class=True)
        assert ent == ref and list(ent[4]) == list(ref[4])
        assert D.entity_level(got) == get_ner_fmeasure(gold, pred, i2s=I2S)


def _random_seq(rng, n, dense=True):
    w = np.array([2, 3, 4, 3, 4, 2, 3, 1, 1], float) if dense else np.array([12, 2, 2, 2, 2, 1, 1, 1, 1], float)
    gold = rng.choice(9, size=n, p=w / w.sum())
    pred = np.where(rng.rand(n) < 0.75, gold, rng.choice(9, size=n, p=w / w.sum()))
    return list(pred), list(gold)


def _random_batches(rng, n_adds, B, L, p_empty=0.2, dense=True):
    out = []
    for _ in range(n_adds):
        seqs = [_random_seq(rng, 0 if rng.rand() < p_empty else int(rng.randint(1, L + 1)), dense) for _ in range(B)]
        out.append(_batch(seqs, L))
    return out


def _planted():
    """4 adds at B = 7, L = 12, ragged"""
    rng = np.random.RandomState(5)
    E, R = ([], []), lambda n: _random_seq(rng, n)
    same = lambda *ids: (list(ids), list(ids))
    adds = [
        [E,                                                   # a zero-length sequence first
         same(O, Ba, Ia), same(Ia, Ia, O),                    # a span across a sequence boundary: a match
         E,                                                   # ... in the middle
         ([Bb, Ib, O, O], [Bb, O, O, O]),                     # a candidate that dies inside a sequence
         same(O, O, Bc),                                      # opens a candidate at the end of the batch's last token
         E],                                                  # ... and last
        [E, same(Ic, Ic, O),                                  # the span runs on across the batch boundary (and two empty sequences)
         same(O, Ba), ([Ia, O], [O, O]),                      # a candidate that dies at a sequence boundary
         R(12), R(7), same(PAD, Bb)],                         # opens one at the batch's end
        [([O, Bb], [Ib, Bb]),                                 # ... which dies at the batch boundary (gold's span runs on)
         R(12), E, R(1), R(12), E, R(5)],
        [R(12), E, R(3), R(12), same(O, O), same(O, Bb, Ib), E],      # a match still open at the end of the stream
    ]
    return [_batch(s, 12) for s in adds]


def _spans(ids):
    from re2nn_seq_amd.metrics.metrics import bio_spans
    T = _tables()
    return list(zip(*(a.tolist() for a in bio_spans(ids, T.kind, T.type))))


def test_planted_stream_cases():
    from re2nn_seq_amd.metrics import device as D
    batches = _planted()
    assert all(t.shape == (7, 12) for t, _, _ in batches) and len(batches) == 4
    # ---- on the CPU, with metrics.py: each planted case is there
    pred, gold = _flat(batches)
    lens = np.concatenate([ln for _, _, ln in batches])
    seq_start = np.concatenate([[0], np.cumsum(lens)])                       # flat index where each sequence starts
    batch_start = seq_start[::7][:4]
    assert all(0 in ln and len(set(ln.tolist())) > 2 for _, _, ln in batches)          # ragged, every add
    assert batches[0][2][0] == 0 and batches[0][2][3] == 0 and batches[0][2][6] == 0
    ps, gs = _spans(pred), _spans(gold)
    joint = set(ps) & set(gs)
    inner = set(seq_start[1:-1].tolist()) - set(batch_start.tolist())
    crosses = lambda s, e, cuts: any(s < c <= e for c in cuts)
    assert any(e >= 0 and crosses(s, e, inner) for s, e, _ in joint), 'no matched span across a sequence boundary'
    assert any(e >= 0 and crosses(s, e, batch_start[1:]) for s, e, _ in joint), 'no matched span across a batch boundary'
    ends = lambda spans: {(s, t): e for s, e, t in spans}
    pe, ge = ends(ps), ends(gs)
    dies_at = [s for (s, t) in pe if (s, t) in ge and pe[(s, t)] != ge[(s, t)] and s + 1 in seq_start]
    assert any(s + 1 in inner for s in dies_at), 'no candidate that dies at a sequence boundary'
    assert any(s + 1 in batch_start for s in dies_at), 'no candidate that dies at a batch boundary'
    assert any(e == -1 for _, e, _ in joint), 'no match open at the end of the stream'
    # ---- scoring the batches one by one and summing differs: a kernel without the carry cannot pass
    T = _tables()
    whole = D.counts_from_flat(pred, gold, T)
    parts = [D.counts_from_flat(*_flat([b]), T) for b in batches]
    assert sum(p.matches for p in parts) != whole.matches
    assert [sum(p.type_match[t] for p in parts) for t in range(3)] != whole.type_match
    # ---- the device
    got = _run(_score(), batches)
    assert got.errors == 0                                                  # (the padding was never read)
    _assert_all_equal(got, batches)


def test_twenty_random_dense_streams():
    rng = np.random.RandomState(11)
    score = _score()
    for _ in range(20):
        batches = _random_batches(rng, 4, 7, 12)
        score.reset()
        _assert_all_equal(_run(score, batches), batches)


@pytest.mark.parametrize('L', [63, 64, 65, 129])
def test_sequence_lengths_around_the_64_positions_of_a_pass(L):
    rng = np.random.RandomState(L)
    full = lambda n: _random_seq(rng, n)
    # full rows (a link across the pass boundary at 64 is likely in a dense mix), a one-token row, and ragged ones
    batches = [_batch([full(L), full(1), full(L)], L), _batch([full(L - 1), full(L), full(min(L, 64))], L),
               _batch([([Ba] + [Ia] * (L - 1), [Ba] + [Ia] * (L - 1)), ([Ia] * L, [Ia] * L), ([Ia] * 2 + [O], [Ia] * 3)], L)]
    _assert_all_equal(_run(_score(), batches), batches)


def _sequences_in_flight():
    from re2nn_seq_amd import _lib
    return _lib.SCORE_WAVES


@pytest.mark.parametrize('B', [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129])
def test_batch_sizes_around_the_sequences_in_flight_and_the_resolving_pass(B):
    """SCORE_WAVES = 16 sequences are in flight (one per wavefront), 64 per pass of the offset scan and of the resolution"""
    assert _sequences_in_flight() == 16
    rng = np.random.RandomState(B)
    batches = _random_batches(rng, 2, B, 5, p_empty=0.3) + _random_batches(rng, 1, B, 5, p_empty=0.9)
    # a span over many sequences: every first token continues the sequence before it
    run = [([Ba, Ia], [Ba, Ia])] + [([Ia], [Ia])] * (B - 1)
    batches.append(_batch(run, 5))
    _assert_all_equal(_run(_score(), batches), batches)


def test_an_add_of_empty_sequences_changes_nothing():
    rng = np.random.RandomState(3)
    batches = _random_batches(rng, 2, 7, 12)
    score = _score()
    before = _run(score, batches)
    empty = _batch([([], [])] * 7, 12)
    after = _run(score, [empty])
    assert after.integers() == before.integers() and after.adds == 3
    more = _random_batches(rng, 1, 7, 12)
    got = _run(score, more)
    assert got.integers() == _want(batches + more).integers()


def _want(batches):
    from re2nn_seq_amd.metrics import device as D
    return D.counts_from_flat(*_flat(batches), _tables())


def test_ids_outside_the_tables_are_counted_and_index_nothing():
    seqs = [([Ba, 99, Ia, O], [Ba, Ia, Ia, O]), ([Bb, Ib, -3, Bc], [Bb, Ib, Ib, Bc]), ([O, Bc], [2 ** 40, Bc])]
    batches = [_batch(seqs, 6)]
    got = _run(_score(), batches)
    assert got.errors == 3
    assert got.integers() == _want(batches).integers()


def test_reset_and_determinism():
    rng = np.random.RandomState(8)
    batches = _random_batches(rng, 4, 7, 12)
    score = _score()
    first = _run(score, batches)
    score.reset()
    again = _run(score, batches)
    other = _run(_score(), batches)
    assert first.integers() == again.integers() == other.integers() == _want(batches).integers()
    assert first.adds == again.adds == 4 and first.loss_sum == again.loss_sum == 0.0


def test_the_loss_sum_is_pythons_double_sum_bit_for_bit():
    rng = np.random.RandomState(2)
    batches = _random_batches(rng, 6, 3, 5)
    host = (rng.rand(6) * 10.0 ** rng.randint(-3, 4, size=6)).astype(np.float32)
    losses = [torch.tensor(float(v), dtype=torch.float32, device='cuda:0') for v in host]
    got = _run(_score(), batches, losses)
    want = 0.0
    for t in losses:
        want += float(t)
    assert got.loss_sum == want and got.loss_sum.hex() == want.hex()
    assert want != float(np.sum(host, dtype=np.float32))                    # (a float32 sum would differ: the test sees the difference)


# ---- through the command line: the switch off and on ---------------------------------------------------------------------
MODELS = {                   # the five trainable mirrors: (--method, --independent, automaton, the step's own opt-in)
    'onehot-ifst': ('onehot', '2', 'ID2', None), 'onehot-fst': ('onehot', '0', 'ID0', 'RE2NN_ONEHOT_FST_TRAIN'),
    'onehot-ind1': ('onehot', '1', 'ID1', 'RE2NN_ONEHOT_IND1_TRAIN'), 'decomp-ifst': ('decompose', '2', 'IIID', None),
    'decomp-ind1': ('decompose', '1', 'IID', 'RE2NN_DECOMP_IND1_TRAIN'),
}


def _tree(tmp_path):
    from re2nn_seq_amd import synth
    return synth.write_dataset_tree(str(tmp_path / 'data'), dataset='ATIS-BIO', seed=4)


def _cli_argv(tmp_path, model):
    """as tests/test_gpu_ind1_train.py::_cli_argv builds it: --bz 9 --seq_max_len 12 --epoch 2"""
    method, independent, automaton, _ = MODELS[model]
    tree = _tree(tmp_path)
    argv = ['--dataset', 'ATIS-BIO', '--method', method, '--independent', independent, '--automata_path', tree['paths'][automaton],
            '--normalize_automata', 'none', '--rand_constant', '0', '--bz', '9', '--seq_max_len', '12',
            '--epoch', '2', '--lr', '0.01', '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir']]
    if method == 'decompose':
        argv += ['--rank', '100', '--seed', '1', '--beta', '0.9', '--embed_dim', '16', '--update_nonlinear', 'tanh']
        if independent == '1':
            argv += ['--rank_wildcard', '70']
    return argv


def _cli_run(tmp_path, monkeypatch, model, switch):
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd.metrics import device as D
    from re2nn_seq_amd.tools.printer import Best_Model_Recorder
    states, reads = [], []
    record = Best_Model_Recorder.update_and_record
    read = D.DeviceScore.read

    def spy_record(self, res_train, res_dev, res_test, sd):
        states.append({k: (v.detach().cpu().numpy().copy() if torch.is_tensor(v) else np.array(v)) for k, v in sd.items()})
        return record(self, res_train, res_dev, res_test, sd)

    def spy_read(self):
        c = read(self)
        reads.append(c.n)
        return c
    with monkeypatch.context() as m:                          # (undone at the end: the next run spies on the real methods)
        if switch:
            m.setenv('RE2NN_DEVICE_METRICS', '1')
        else:
            m.delenv('RE2NN_DEVICE_METRICS', raising=False)
        if MODELS[model][3]:
            m.setenv(MODELS[model][3], '1')
        m.setattr(Best_Model_Recorder, 'update_and_record', spy_record)
        m.setattr(D.DeviceScore, 'read', spy_read)
        results, stats, res_path = cli.main(_cli_argv(tmp_path, model) + ['--model_dir', str(tmp_path / ('on' if switch else 'off'))])
    saved = cli.load_res(res_path)
    return dict(results=results, record=[line for line in saved['logger'].record if 'THROUGHPUT' not in line],
                throughput=sum('THROUGHPUT' in line for line in saved['logger'].record),
                res={k: getattr(saved['res'], k) for k in ('best_dev_results', 'best_dev_train_results', 'best_dev_test_results',
                                                           'best_selector')},
                states=states, reads=reads)


@pytest.mark.parametrize('model', ['onehot-ifst', 'onehot-fst', 'onehot-ind1', 'decomp-ind1'])
def test_cli_logs_results_and_weights_are_equal_with_the_switch_off_and_on(tmp_path, monkeypatch, model):
    """The four mirrors whose step is bit-identical across runs (include/farnn.h: no float atomics): everything but the THROUGHPUT
    lines is equal string for string, and so are the saved results and the weights after each epoch."""
    off = _cli_run(tmp_path, monkeypatch, model, False)
    on = _cli_run(tmp_path, monkeypatch, model, True)
    assert off['reads'] == [] and len(on['reads']) >= 2 and all(n > 0 for n in on['reads'])      # the scorer ran, and only when asked
    assert len(off['record']) > 8 and any('LOSS:' in line for line in off['record'])
    assert on['record'] == off['record']
    assert on['throughput'] == off['throughput']
    assert on['results'] == off['results'] and on['res'] == off['res']
    assert len(on['states']) == len(off['states']) == 2
    for a, b in zip(on['states'], off['states']):
        assert list(a) == list(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_cli_of_the_decomposed_ifst_logs_what_metrics_py_gives_for_its_own_steps(tmp_path, monkeypatch):
    """The decomposed i-FST's step adds its loss and gradients with float atomics (csrc/train.hip.h): two runs of the SAME code
    differ in the last bits, so no off/on comparison of two runs can be string for string.  Its run with the switch on is held to
    metrics.py within the run instead: every step's loss, tags, labels and lengths are recorded as the step returns them, and
    the logged LOSS line and the TRAIN results of each epoch must equal Python's double sum and metrics.py on the flat lists."""
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import train_onehot
    from re2nn_seq_amd.farnn._trainable import Trainable
    from re2nn_seq_amd.metrics.metrics import eval_seq_token, get_ner_fmeasure
    steps, logged = [], []
    real_step, real_log = Trainable.forward_local_device, train_onehot.print_and_log_results

    def spy_step(self, *a, **k):
        out = real_step(self, *a, **k)
        steps.append([t.detach().cpu() for t in out])
        return out

    def spy_log(logger, res, epoch, mode):
        logged.append((mode, epoch, res))
        return real_log(logger, res, epoch, mode)
    monkeypatch.setenv('RE2NN_DEVICE_METRICS', '1')
    monkeypatch.setattr(Trainable, 'forward_local_device', spy_step)
    monkeypatch.setattr(train_onehot, 'print_and_log_results', spy_log)
    _, _, res_path = cli.main(_cli_argv(tmp_path, 'decomp-ifst') + ['--model_dir', str(tmp_path / 'on')])
    saved = cli.load_res(res_path)
    dset = _tree(tmp_path)['dset']
    i2s, o_idx, n_train = dset['i2s'], dset['s2i']['o'], len(dset['query_train'])

    def flatten(t, ln):
        return torch.from_numpy(t.numpy()[np.arange(t.shape[1])[None, :] < ln.numpy()[:, None]].astype(np.int64))
    losses = [line for line in saved['logger'].record if 'LOSS:' in line]
    train = [res for mode, epoch, res in logged if mode == 'TRAIN' and epoch != 'INIT']
    assert len(steps) % 2 == 0 and len(steps) >= 4 and len(losses) == len(train) == 2
    per = len(steps) // 2
    for e in range(2):
        mine = steps[e * per:(e + 1) * per]
        total = 0.0
        for loss, _, _, _ in mine:
            total += float(loss)
        assert losses[e].strip() == 'TRAIN Epoch: {} | LOSS: {}'.format(e + 1, total / n_train)
        pred = torch.cat([flatten(t, ln) for _, t, _, ln in mine])
        gold = torch.cat([flatten(g, ln) for _, _, g, ln in mine])
        assert train[e] == {'token-level': list(eval_seq_token(pred, gold, o_idx=o_idx)),
                            'entity-level': list(get_ner_fmeasure(gold, pred, i2s=i2s))}


def test_val_onehot_returns_an_equal_dict_on_the_host_path_and_with_the_scorer(tmp_path, monkeypatch):
    """an onehot i-FST as the command line builds it, evaluated on the three splits: the pinned-buffer pipeline (what runs with or
    without the switch) against device_metrics=True"""
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import train_onehot, val
    from re2nn_seq_amd.data import iter_batches
    argv = _cli_argv(tmp_path, 'onehot-ifst')
    argv[argv.index('--epoch') + 1] = '0'
    got = {}
    real = train_onehot.init_evaluation

    def spy(model, splits, args, s2i, i2s, logger, model_dir='../model_seq/'):
        got.update(model=model, splits=splits, args=args, s2i=s2i, i2s=i2s)
        return real(model, splits, args, s2i, i2s, logger, model_dir)
    made = []
    real_score = val._device_score

    def spy_score(*a, **k):
        made.append(real_score(*a, **k))
        return made[-1]
    monkeypatch.setattr(train_onehot, 'init_evaluation', spy)
    monkeypatch.setattr(val, '_device_score', spy_score)
    monkeypatch.setenv('RE2NN_DEVICE_METRICS', '1')
    results, _, _ = cli.main(argv + ['--model_dir', str(tmp_path / 'm')])
    assert made == []                                        # the switch alone leaves evaluation on the host path
    for split in ('train', 'dev', 'test'):
        batches = lambda: iter_batches(got['splits'][split], got['args'].bz)
        host = val.val_onehot(batches(), got['model'], got['args'], got['s2i']['o'], got['i2s'])
        dev = val.val_onehot(batches(), got['model'], got['args'], got['s2i']['o'], got['i2s'], device_metrics=True)
        assert dev == host == results[split]
        assert list(dev['entity-level'][4]) == list(host['entity-level'][4])
    assert len(made) == 3 and all(s is not None for s in made)
