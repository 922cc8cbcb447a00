"""The long reads of tools/any_timing.py (diagonals of 65 .. 4096 intervals on one chromosome, two per length)
through the 'pairs' engine: at overlap 0.0 every same-chromosome cell matches, and k_cap_eval decides the 45
pairs over the whole lists.  Three queries; the kernel's time comes from a kernel trace around the run:

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/pairs_timing.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from fslr_amd import _lib, cluster            # noqa: E402
from match_ref import resident_data           # noqa: E402


def diag(n, shift=0):
    return [(1, 10_000 * k + shift, 10_000 * k + shift + 1000, 1000) for k in range(n)]


lens = [65, 130, 300, 1000, 4096]
reads = [diag(Ln, 5 * (t % 2)) for Ln in lens for t in range(2)]
data = resident_data(reads, [1000] * len(reads), [4] * len(reads))
ctx = _lib.Context(0)
idx = cluster.build_interval_trees(data, ctx=ctx)
for rep in range(3):
    g = cluster.query_graph(idx, data, 0.0, [0.01], 10, 0.04, 0.25)
    edges = sorted(zip(g.a.tolist(), g.b.tolist(), g.I.tolist(), g.U.tolist()))
    print(g.stats['engine'], len(edges), edges[:3], flush=True)
ctx.close()
