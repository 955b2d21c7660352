"""Evaluation loop over a dataset: the caller of the hot path (reference src_seq/val.py:7-43).

Same signature and result dict as the reference's ``val_onehot``.  The reference appends every
predicted token to a Python list as a 0-d tensor and scores them in pure-Python loops; here the
flat predictions stay tensors until one concatenation, and the metrics are vectorised."""
import collections
import time

import torch

from .data import iter_batches
from ._lib import MODE_LOCAL
from .metrics.device import DeviceScore, entity_level, token_level
from .metrics.metrics import eval_seq_token, get_ner_fmeasure


def _device_score(model, o_idx, i2s):
    """A DeviceScore for an evaluation that asked for one, where the model tags on the device and the label map has integer tables
    (metrics._label_tables); None otherwise: the host path runs as it always has."""
    if i2s is None:
        return None
    if not (hasattr(model, 'run') and hasattr(model, '_dev')) or not DeviceScore.supported(i2s):
        return None
    model.handle                                  # (no device, no handle: the same error as the host path's)
    return DeviceScore(i2s, o_idx, model._dev())


def val_onehot(dataloader, model, args, o_idx=0, i2s=None, i2t=None, is_cuda=True, stats=None, device_metrics=False):
    """`dataloader`: any iterable of {'x','s','l'} batches (a torch DataLoader, or a dataset from
    data.py which is then batched with args.bz).  `stats` (optional dict) receives timing.
    `device_metrics`: tag with run(..., MODE_LOCAL, want_tags=True) and count on the device (metrics/device.py), one read at the
    end.  Equal results, but measured SLOWER than the pinned-buffer pipeline at the headline shape, so no
    caller asks for it: RE2NN_DEVICE_METRICS=1 leaves evaluation on the host path; scripts/time_device_metrics.py times both."""
    if hasattr(dataloader, '__getitem__') and not hasattr(dataloader, '__iter__'):
        dataloader = iter_batches(dataloader, args.bz)
    preds, trues = [], []
    n_tok, t0 = 0, time.perf_counter()
    model.eval()
    # the reference calls forward_local and reads the result batch by batch (val.py:28-31); here up to
    # `pipeline_depth` batches are in flight: the H2D copy and launch of batch i+1 are enqueued before the
    # predictions of batch i-1 are read back (same calls, same order of results)
    submit = getattr(model, 'submit_local', None)
    depth = getattr(model, 'pipeline_depth', 0) if submit is not None and not getattr(model, 'training', False) else 0
    pending = collections.deque()
    score = _device_score(model, o_idx, i2s) if device_metrics else None

    def collect(item):
        _, pred_label, true_label = item.result()
        preds.append(pred_label.reshape(-1).cpu())
        trues.append(true_label.reshape(-1).cpu())

    with torch.no_grad():
        for batch in dataloader:
            x, label, lengths = batch['x'], batch['s'], batch['l']
            if score is not None:
                x = model._clip_len(x, lengths)
                r = model.run(x, lengths, MODE_LOCAL, want_tags=True)
                score.add(r['tags'], label[:, :x.shape[1]], r['_keep'][1])
            elif depth > 0:
                pending.append(submit(x, label, lengths))
                if len(pending) > depth:
                    collect(pending.popleft())
            else:
                _, pred_label, true_label = model.forward_local(x, label, lengths, train=False)
                preds.append(pred_label.reshape(-1).cpu())
                trues.append(true_label.reshape(-1).cpu())
            n_tok += int(lengths.sum())
        while pending:
            collect(pending.popleft())
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    counts = score.read() if score is not None else None
    elapsed = time.perf_counter() - t0
    if counts is not None and counts.n > 0:
        if counts.errors:
            raise ValueError('{} tags or labels outside the label map reached the device scorer'.format(counts.errors))
        if stats is not None:
            stats.update(tokens=n_tok, seconds=elapsed, tokens_per_s=n_tok / elapsed if elapsed > 0 else 0.0)
        model.train()
        return {'token-level': list(token_level(counts)), 'entity-level': list(entity_level(counts, all_class=True))}
    all_pred = torch.cat(preds) if preds else torch.zeros(0, dtype=torch.int64)
    all_true = torch.cat(trues) if trues else torch.zeros(0, dtype=torch.int64)
    acc, p, r, f = eval_seq_token(seq_label_pred=all_pred, seq_label_true=all_true, o_idx=o_idx)
    acc_ner, p_ner, r_ner, f_ner, class_res = get_ner_fmeasure(
        golden_lists=all_true, predict_lists=all_pred, label_type="BIO", i2s=i2s, all_class=True)
    if stats is not None:
        stats.update(tokens=n_tok, seconds=elapsed, tokens_per_s=n_tok / elapsed if elapsed > 0 else 0.0)
    model.train()
    return {'token-level': [acc, p, r, f],
            'entity-level': [acc_ner, p_ner, r_ner, f_ner, class_res]}
