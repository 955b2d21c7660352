#!/usr/bin/env python3
"""Golden fixture for the layout the reference's D.automata writer decomposes (src_seq/wfa/fsa_to_tensor.py:176-257,
dfa_to_tensor_slot_new): C = len(slot2idx) with no `oo` column, '$<:>oo' edges in wildcard_wildcard_tensor[S,S], '$' edges with a
slot in wildcard_tensor[C,S,S], word and class ('&', '%') edges in language_tensor[V,C,S,S], an out-of-vocabulary rule word
nowhere.  Runs only where the reference is present (imports its loader):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fst_new.py <reference checkout>

Input: the automaton of loader_small.json plus the edges listed in EXTRA_EDGES (also applied by the test).
Output: tests/golden/fst_new_small.npz (data only: the resulting arrays and the sorted language list)."""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

# (from, to, 'word<:>slot'): two words outside the vocabulary, and one edge of every kind the layout tells apart, so that the
# fixture has them whatever loader_small.json holds
EXTRA_EDGES = [(0, 1, 'notaword<:>b-e1'), (2, 3, 'alsomissing<:>i-e2'), (1, 2, '&<:>b-e1'), (2, 1, '%<:>i-e2'), (3, 2, '$<:>b-e1'),
               (1, 1, '$<:>oo')]


def automaton_with_extras():
    with open(os.path.join(HERE, 'loader_small.json')) as f:
        meta = json.load(f)
    a = meta['automaton']
    automaton = {'states': set(a['states']), 'startstate': a['startstate'], 'finalstates': a['finalstates'],
                 'transitions': {int(fr): {int(to): set(e) for to, e in d.items()}
                                 for fr, d in a['transitions'].items()}}
    for fr, to, lab in EXTRA_EDGES:
        automaton['transitions'].setdefault(fr, {}).setdefault(to, set()).add(lab)
    return automaton, meta['t2i'], meta['s2i']


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit('usage: make_golden_fst_new.py <checkout of the reference (the directory that holds src_seq/)>')
    sys.path.insert(0, sys.argv[1])
    from src_seq.wfa import fsa_to_tensor as ref_f2t
    automaton, t2i, s2i = automaton_with_extras()
    with contextlib.redirect_stdout(io.StringIO()):
        r = ref_f2t.dfa_to_tensor_slot_new(automaton, t2i, s2i)
    out = {'language_tensor': r[0], 'wildcard_tensor': r[2], 'wildcard_wildcard_tensor': r[3], 'final_vector': r[4],
           'start_vector': r[5], 'language': np.array(sorted(r[6]))}
    np.savez_compressed(os.path.join(HERE, 'fst_new_small.npz'), **out)
    print('wrote fst_new_small.npz', {k: v.shape for k, v in out.items()},
          {k: int(np.count_nonzero(v)) for k, v in out.items() if k != 'language'})
