#!/usr/bin/env python3
"""Records tests/golden/planning_info_parent.json: every output of `engine.colloc_band_info` and `engine.colloc_elimination_info`
over a grid of plan shapes, from the library and binding of the tree this script stands in (host arithmetic, needs no GPU).

    python tests/golden/make_planning_info.py [OUT.json]

The fixture was recorded with the commit BEFORE the planning entry points' host code was restated (one pair parser, one shape
filler, one routing rule); tests/test_planning_info.py holds every later build to it, field by field, as integers.  A case
holds its own arguments, so the test runs what the file lists.  A refused call is recorded with the library's text.

The grid: 1 to 4 vehicles; strategy lengths from {2, 3, 11, 52, 53} (at five intervals per step 52 steps are 255 intervals, 53 are
260: the two sides of the structured elimination's eight-bit interval count), mixed vectors among them, [53, 3] the joint plan
that one long vehicle sends to the band; terminal headings all given and mixed; 0, 4, 6, 8 obstacles; all pairs, a subset, none;
both eliminations."""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

N_SETS = ([2], [3], [11], [52], [53],
          [3, 2], [11, 7], [53, 3], [52, 52], [2, 53],
          [11, 7, 7], [3, 2, 3], [52, 3, 2], [2, 53, 3],
          [11, 7, 7, 9], [2, 2, 2, 2], [3, 52, 2, 11], [3, 53, 2, 11])
N_OBS = (0, 4, 6, 8)
MIXED_FINAL = [1, 0, 0, 1]


def pair_choices(V):
    """None (all pairs), a subset given explicitly, the empty list."""
    return (None, [[0, 2]] if V > 2 else [[0, 1]] if V == 2 else [], []) if V > 1 else (None, [])


def grid():
    for ns in N_SETS:
        for hf, n_obs, pairs in itertools.product((None, MIXED_FINAL[:len(ns)]), N_OBS, pair_choices(len(ns))):
            yield dict(n_sets=list(ns), has_final=hf, n_obs=n_obs, pairs=pairs)


def record(engine, case):
    """The case with what the two entry points answer: band [nk, kb, band_bytes], elim [structured 0, structured 1]."""
    def call(f, **kw):
        try:
            r = f(case["n_sets"], n_obs=case["n_obs"], pairs=case["pairs"], has_final=case["has_final"], **kw)
        except RuntimeError as e:
            return {"error": str(e)}
        return list(r) if isinstance(r, tuple) else r

    return dict(case, band=call(engine.colloc_band_info), elim=[call(engine.colloc_elimination_info, structured=s) for s in (0, 1)])


def main():
    from conflict_rez_amd import engine

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "planning_info_parent.json")
    cases = [record(engine, c) for c in grid()]
    with open(out, "w") as f:
        f.write('{"N_per_set": 5, "cases": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]}\n")
    print(f"{out}: {len(cases)} cases, {sum('error' in c['band'] for c in cases)} refused")


if __name__ == "__main__":
    main()
