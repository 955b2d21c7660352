"""The scores of metrics.py from COUNTS, and the device-side counter of them (include/farnn.h farnn_score_*).

metrics.py scores one flat list per data set.  Everything eval_seq_token and get_ner_fmeasure return is a ratio of a dozen
integers over that list (per type: three more and two first positions), so the list itself need not reach the host: DeviceScore
counts it on the device, one launch per batch, and is read once.  token_level() / entity_level() turn the counts into metrics.py's
tuples with its own expressions (the -1 and 0 conventions and the per_class key order included); counts_from_flat() is the numpy
restatement of the counting rule, for tests without a device.

The span matches are counted in streaming form.  With `prev` the previous token of the list, link[j] = kind[j] == 2 and
kind[prev] != 0 and type[j] == type[prev] (for pred and gold separately; bio_spans' link).  A position where pred and gold are
both B- of one type opens a candidate; it is a match at the next position where both links are false, dies at the next position
where exactly one is false, and is a match if the list ends first."""
import numpy as np

from .metrics import _label_tables

_INT_FIELDS = ('n', 'same', 'canon_same', 'tp', 'fp', 'fn', 'pred_spans', 'gold_spans', 'matches', 'errors')
_TYPE_FIELDS = ('type_pred', 'type_gold', 'type_match', 'first_pred', 'first_gold')


class Tables:
    """Per label id: kind (0 other, 1 B-, 2 I-), type and canon (the first id with the same spelling: get_ner_fmeasure compares
    label strings, metrics.py:131-134); names[type]; o_idx."""

    def __init__(self, kind, type_, canon, names, o_idx):
        self.kind, self.type, self.canon = (np.asarray(a, np.int64) for a in (kind, type_, canon))
        self.names, self.o_idx = list(names), int(o_idx)


def label_tables(i2s, o_idx):
    """Tables of a label map, or None where metrics._label_tables gives None (a B- label with an empty type)."""
    t = _label_tables(i2s)
    if t is None:
        return None
    kind, typ, names = t
    spell, canon = {}, np.arange(len(kind))
    for k, raw in i2s.items():
        canon[int(k)] = spell.setdefault(raw, int(k))
    return Tables(kind, typ, canon, names, o_idx)


class Counts:
    """Plain counts of one flat list: the integers of _INT_FIELDS, loss_sum (a double) and adds, per type the lists of
    _TYPE_FIELDS (first_*: the flat index of the type's first B-, -1 if none), and names[type]."""

    def __init__(self, names, **kw):
        self.names = list(names)
        for f in _INT_FIELDS:
            setattr(self, f, int(kw.get(f, 0)))
        self.adds, self.loss_sum = int(kw.get('adds', 0)), float(kw.get('loss_sum', 0.0))
        for f in _TYPE_FIELDS:
            setattr(self, f, [int(v) for v in kw.get(f, [0 if f.startswith('type') else -1] * len(self.names))])

    def integers(self):
        """Every count but adds and loss_sum, as one comparable dict."""
        return {f: getattr(self, f) for f in _INT_FIELDS + _TYPE_FIELDS}


def counts_from_flat(pred, gold, tables):
    """The counts of a flat list by the streaming rule above, in numpy.  An id outside the tables is kind 0, compares as its raw
    value and counts in `errors` (as the device does)."""
    pred, gold = np.asarray(pred, np.int64).ravel(), np.asarray(gold, np.int64).ravel()
    assert len(pred) == len(gold)
    n, nl, nt, o = len(pred), len(tables.kind), len(tables.names), tables.o_idx

    def look(ids):
        ok = (ids >= 0) & (ids < nl)
        safe = np.where(ok, ids, 0)
        return ok, np.where(ok, tables.kind[safe], 0), np.where(ok, tables.type[safe], -1), np.where(ok, tables.canon[safe], ids)

    def links(kind, typ):
        link = np.zeros(n, bool)
        link[1:] = (kind[1:] == 2) & (kind[:-1] != 0) & (typ[1:] == typ[:-1])
        return link
    okp, kp, tp_, cp = look(pred)
    okg, kg, tg, cg = look(gold)
    lp, lg = links(kp, tp_), links(kg, tg)
    same = pred == gold
    out = dict(n=n, same=same.sum(), canon_same=(cp == cg).sum(), tp=(same & (pred != o)).sum(), fp=(~same & (pred != o)).sum(),
               fn=(~same & (gold != o)).sum(), pred_spans=(kp == 1).sum(), gold_spans=(kg == 1).sum(), errors=(~(okp & okg)).sum())
    # a candidate lives from the event that opens it to the very next event (a position where not both links hold)
    events = np.nonzero(~(lp & lg))[0]
    both = ~lp[events] & ~lg[events]
    opens = np.where((kp == 1) & (kg == 1) & (tp_ == tg), tp_, -1)[events]
    closed_by_match = np.append(both[1:], True)              # the list's end closes the last one as a match
    hit = opens[(opens >= 0) & closed_by_match]
    out['matches'] = len(hit)
    out['type_match'] = np.bincount(hit, minlength=nt)
    for name, k, t in (('pred', kp, tp_), ('gold', kg, tg)):
        starts = np.nonzero((k == 1) & (t >= 0))[0]
        out['type_' + name] = np.bincount(t[starts], minlength=nt)
        first = np.full(nt, -1, np.int64)
        first[t[starts][::-1]] = starts[::-1]                 # (the earliest start of a type is written last)
        out['first_' + name] = first
    return Counts(tables.names, **out)


def token_level(c):
    """eval_seq_token's (accuracy, precision, recall, f1) (metrics.py:17-28)."""
    tp, fp, fn = c.tp, c.fp, c.fn
    accuracy = float(c.same) / c.n
    precision = tp / (tp + fp) if (tp + fp) else 0
    recall = tp / (tp + fn) if (tp + fn) else 0
    f1 = 2 * precision * recall / (precision + recall) if (precision + recall) else 0
    return accuracy, precision, recall, f1


def _prf(right, n_pred, n_gold):
    precision = right / n_pred if n_pred else -1
    recall = right / n_gold if n_gold else -1
    if precision == -1 or recall == -1 or (precision + recall) <= 0.:
        return precision, recall, -1
    return precision, recall, 2 * precision * recall / (precision + recall)


def entity_level(c, all_class=False):
    """get_ner_fmeasure's (accuracy, precision, recall, f_measure, per_class) (metrics.py:121-157).  per_class keys in the order of
    first appearance: the types with a pred span by their first pred start, then those seen in gold only by their first gold start."""
    accuracy = float(c.canon_same) / c.n
    precision, recall, f_measure = _prf(c.matches, c.pred_spans, c.gold_spans)
    per_class = None
    if all_class:
        nt = range(len(c.names))
        order = sorted((t for t in nt if c.type_pred[t]), key=lambda t: c.first_pred[t]) + \
            sorted((t for t in nt if c.type_gold[t] and not c.type_pred[t]), key=lambda t: c.first_gold[t])
        per_class = {c.names[t]: list(_prf(c.type_match[t], c.type_pred[t], c.type_gold[t])) for t in order}
    return accuracy, precision, recall, f_measure, per_class


class DeviceScore:
    """The counts of one flat list, kept on the device.  add() enqueues one launch on the current stream of `device` and waits for
    nothing; read() waits once and returns Counts.  The adds of one DeviceScore must be ordered on one stream."""

    def __init__(self, i2s, o_idx, device=0):
        from .. import _lib
        self.tables = label_tables(i2s, o_idx)
        if self.tables is None:
            raise ValueError('a B- label with an empty type: this label map is scored on the host (metrics._label_tables)')
        import torch
        self._dev = device if isinstance(device, torch.device) else torch.device('cuda', int(device))
        t = self.tables
        self._score = _lib.Score(t.kind, t.type, t.canon, len(t.names), t.o_idx, device=self._dev.index or 0)

    @staticmethod
    def supported(i2s):
        return _label_tables(i2s) is not None

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self._dev).cuda_stream

    def add(self, tags, labels, lengths, loss=None):
        """tags int32 [B, L], labels int64 [B, L], lengths int64 [B], loss a float32 scalar or None: tensors on the device (anything
        else is converted there first)."""
        import torch
        dev = self._dev
        tags = tags.to(device=dev, dtype=torch.int32).contiguous()
        labels = labels.to(device=dev, dtype=torch.int64).contiguous()
        lengths = lengths.to(device=dev, dtype=torch.int64).contiguous()
        B, L = tags.shape
        if tuple(labels.shape) != (B, L) or tuple(lengths.shape) != (B,):
            raise ValueError('tags [B, L], labels [B, L] and lengths [B] do not agree: {} {} {}'.format(
                tuple(tags.shape), tuple(labels.shape), tuple(lengths.shape)))
        if loss is not None:
            loss = loss.detach().to(device=dev, dtype=torch.float32).reshape(-1)[:1].contiguous()
        with torch.cuda.device(dev):
            self._score.add(tags.data_ptr(), labels.data_ptr(), lengths.data_ptr(), B, L,
                            None if loss is None else loss.data_ptr(), self._stream())
        self._keep = (tags, labels, lengths, loss)            # until the next add: the launch may not have run yet

    def read(self):
        import torch
        with torch.cuda.device(self._dev):
            c, per_type = self._score.read(self._stream())
        self._keep = None
        out = {f: getattr(c, f) for f in _INT_FIELDS}
        out.update(zip(_TYPE_FIELDS, per_type))
        return Counts(self.tables.names, adds=c.adds, loss_sum=c.loss_sum, **out)

    def reset(self):
        import torch
        with torch.cuda.device(self._dev):
            self._score.reset(self._stream())
