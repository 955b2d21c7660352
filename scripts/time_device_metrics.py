"""What counting an epoch's loss and tag metrics on the device is worth (RE2NN_DEVICE_METRICS=1), at the
headline training shape of scripts/time_onehot_train.py: the onehot i-FST with V = 950, S = 71, C = 128, batches of B = 256
sequences of L = 64 with ragged lengths, under RE2NN_NATIVE_OPTIM=1.  The label map has 63 BIO types.

  train   train_onehot.train_epochs for one epoch over --batches batches: the seconds of its THROUGHPUT | TRAIN-STEP line (the
          epoch loop up to and including the scores' inputs: with the switch the one read, without it every batch's copies)
  eval    val.val_onehot over the same batches, as it runs (`host`: the pinned-buffer pipeline, with or without the switch) and
          with device_metrics=True (`device`): the seconds it reports (tagging, the copies or the one read; not the ratios)
  add     the scorer's launch alone: HIP events around --inner back-to-back adds of one batch, per add

Switch-off (`host`, the parent's behaviour) and switch-on (`device`) runs alternate inside every repetition, in one process.
Per contender: the median, the interquartile range (the run-to-run spread), min and max over --reps repetitions.  A difference
counts as a gain only above the larger of the two spreads (`gain` > `spread`: `counts`).  Prints one JSON line and writes it to
profiles/device_metrics_timing.json.

    python scripts/time_device_metrics.py [--reps 9] [--batches 60] [--inner 50] [--warmup 2]

Each GPU step of a job script runs it under its own time limit (timeout -k 10 ...)."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, S, C, B, L = 950, 71, 128, 256, 64


def label_map():
    """'o', B-/I- of 63 types, and a second spelling of 'o' as the pad"""
    i2s = {0: 'o', C - 1: '<pad>'}
    for t in range((C - 2) // 2):
        i2s[1 + 2 * t], i2s[2 + 2 * t] = 'B-t{}'.format(t), 'I-t{}'.format(t)
    return i2s


class Rows:
    """what data.iter_batches walks: one {'x', 's', 'l'} per sequence"""

    def __init__(self, x, s, l):
        self.x, self.s, self.l = x, s, l

    def __len__(self):
        return len(self.l)

    def __getitem__(self, i):
        return {'x': self.x[i], 's': self.s[i], 'l': self.l[i]}


def model_args():
    return argparse.Namespace(rand_constant=0.0, train_wildcard=0, train_wildcard_wildcard=0, margin=0.3, threshold=0.5,
                              train_mode='sum', local_loss_func='CE1', use_priority=0, independent=2, update_nonlinear='none',
                              additional_states=0, use_crf=0, random=0, train_h0=0, train_hT=0, farnn=0, marryup_type='none',
                              optimizer='ADAM', lr=1e-3, epoch=1, bz=B, method='onehot')


def build(n_batches):
    from re2nn_seq_amd import synth
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I_S
    rng = np.random.RandomState(1234)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng)
    xs, ls = [], []
    for _ in range(n_batches):
        x, lengths = synth.random_batch(V, B, L, rng)
        xs.append(x)
        ls.append(lengths)
    x, l = np.concatenate(xs).astype(np.int64), np.concatenate(ls).astype(np.int64)
    s = rng.randint(0, C, size=x.shape).astype(np.int64)
    args = model_args()
    model = FARNN_S_O_I_S(T, O, W, np.zeros(S, np.float32), hT, h0, np.eye(C - 1), args, o_idx=0)
    small = Rows(x[:B], s[:B], l[:B])
    return model, args, {'train': Rows(x, s, l), 'dev': small, 'test': small}


def _stats(v):
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return dict(median_s=round(float(med), 6), iqr_s=round(float(q3 - q1), 6), min_s=round(float(min(v)), 6), max_s=round(float(max(v)), 6))


def _verdict(host, device):
    gain, spread = host['median_s'] - device['median_s'], max(host['iqr_s'], device['iqr_s'])
    return dict(gain_s=round(gain, 6), spread_s=round(spread, 6), counts=bool(abs(gain) > spread),
                device_over_host=round(device['median_s'] / host['median_s'], 3))


class _Recorder:
    def update_and_record(self, *a):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--batches', type=int, default=60)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    os.environ['RE2NN_NATIVE_OPTIM'] = '1'
    import torch
    from re2nn_seq_amd import train_onehot
    from re2nn_seq_amd.data import iter_batches
    from re2nn_seq_amd.metrics.device import DeviceScore
    from re2nn_seq_amd.utils import Logger
    from re2nn_seq_amd.val import val_onehot
    model, args, splits = build(a.batches)
    i2s, s2i = label_map(), {'o': 0}
    if not torch.cuda.is_available():
        sys.exit('time_device_metrics.py needs the GPU: a timing taken anywhere else says nothing')

    def switch(on):
        if on:
            os.environ['RE2NN_DEVICE_METRICS'] = '1'
        else:
            os.environ.pop('RE2NN_DEVICE_METRICS', None)

    def epoch(on):
        switch(on)
        stats = {}
        with contextlib.redirect_stdout(io.StringIO()):
            train_onehot.train_epochs(model, splits, args, s2i, i2s, Logger(), _Recorder(), stats)
        return stats['train_step'][-1]['seconds']

    def evaluation(on):
        switch(False)
        st = {}
        with contextlib.redirect_stdout(io.StringIO()):
            res = val_onehot(iter_batches(splits['train'], B), model, args, 0, i2s, stats=st, device_metrics=on)
        return st['seconds'], res

    names = {'host': False, 'device': True}
    for _ in range(a.warmup):
        for on in names.values():
            epoch(on)
            evaluation(on)
    same = evaluation(False)[1] == evaluation(True)[1]
    train = {k: [] for k in names}
    evalu = {k: [] for k in names}
    for _ in range(a.reps):
        for k, on in names.items():
            train[k].append(epoch(on))
        for k, on in names.items():
            evalu[k].append(evaluation(on)[0])
    switch(False)
    # the launch alone
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(7)
    tags = torch.from_numpy(rng.randint(0, C, size=(B, L)).astype(np.int32)).to(dev)
    labels = torch.from_numpy(splits['train'].s[:B]).to(dev)
    lengths = torch.from_numpy(splits['train'].l[:B]).to(dev)
    loss = torch.ones((), device=dev)
    score = DeviceScore(i2s, 0, dev)
    add_us = []
    for r in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            score.add(tags, labels, lengths, loss=loss)
        e1.record()
        torch.cuda.synchronize()
        if r:                                      # (the first repetition warms the launch up)
            add_us.append(1e3 * e0.elapsed_time(e1) / a.inner)
    q1, med, q3 = np.percentile(add_us, [25, 50, 75])
    out = dict(workload='device_metrics', V=V, S=S, C=C, B=B, L=L, batches=a.batches, tokens=int(splits['train'].l.sum()),
               reps=a.reps, optimizer='farnn.optim.Adam', device=torch.cuda.get_device_name(0), eval_results_equal=bool(same))
    out['train_epoch'] = {k: _stats(v) for k, v in train.items()}
    out['train_epoch']['verdict'] = _verdict(out['train_epoch']['host'], out['train_epoch']['device'])
    out['eval_pass'] = {k: _stats(v) for k, v in evalu.items()}
    out['eval_pass']['verdict'] = _verdict(out['eval_pass']['host'], out['eval_pass']['device'])
    out['add'] = dict(us=round(float(med), 2), iqr_us=round(float(q3 - q1), 2), inner=a.inner,
                      note='back-to-back adds on one stream: launch-bound; one workgroup')
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'device_metrics_timing.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
