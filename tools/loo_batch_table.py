#!/usr/bin/env python
"""From the output of alternating `time_loo_batch.py --mode loop` and `--mode batch` runs (files given in the order they ran) to
the table of profiles/loo_batch_ab.txt and the rule of bopt._LOO_BATCH_MIN_H.

A cell (N, H) is batched where every batched run's median beats every loop run's median by more than the larger of the two
spreads (largest minus smallest median of the runs of one kind).  The rule per size is the smallest measured H from which every
measured H is batched; a size with no such H gets NEVER.

    python tools/loo_batch_table.py run1_loop.txt run1_batch.txt run2_loop.txt run2_batch.txt
"""
import re
import sys

NEVER = 10 ** 9


def main():
    cells = {}
    for path in sys.argv[1:]:
        for line in open(path):
            m = re.search(r"\b(loop|batch)\s+N=\s*(\d+) H=\s*(\d+)\s+median\s+([\d.]+) ms", line)
            if m:
                cells.setdefault((int(m.group(2)), int(m.group(3))), {"loop": [], "batch": []})[m.group(1)].append(float(m.group(4)))
    print(f"{'N':>4} {'H':>3}  {'loop medians ms':28s} {'batch medians ms':28s} {'spread':>7}  {'ratio':>6}  batched")
    rule = {}
    for (N, H), c in sorted(cells.items()):
        lo, ba = c["loop"], c["batch"]
        spread = max(max(lo) - min(lo), max(ba) - min(ba))
        win = max(ba) + spread < min(lo)
        rule.setdefault(N, []).append((H, win))
        fmt = lambda v: " ".join(f"{x:8.3f}" for x in v)   # noqa: E731
        print(f"{N:4d} {H:3d}  {fmt(lo):28s} {fmt(ba):28s} {spread:7.3f}  {min(lo) / max(ba):6.2f}  {'yes' if win else 'no'}")
    table = []
    for N, hs in sorted(rule.items()):
        hmin = NEVER
        for H, win in sorted(hs, reverse=True):
            if not win:
                break
            hmin = H
        table.append((N, hmin))
    print("_LOO_BATCH_MIN_H =", tuple(table))


if __name__ == "__main__":
    main()
