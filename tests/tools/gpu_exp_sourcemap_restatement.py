"""tools/gpu_exp_sourcemap.py plus the NumPy restatement's time (tests/sourcemap_restatement.py)
on the same first few Outputs, one JSON line per size (what profiles/sourcemap_exp.jsonl holds).

    python tests/tools/gpu_exp_sourcemap_restatement.py [N ...]          (default: 1e6 1e7)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from nexoclom_amd import Output                                       # noqa: E402
from tests import sourcemap_restatement as R                          # noqa: E402
from tools import gpu_exp_sourcemap as E                              # noqa: E402


def restatement_ms(few):
    outs = []
    for run in few.inputs._catalogue:
        X0 = Output.upcast(run.X0)
        outs.append({c: X0[c].values for c in
                     ('longitude', 'latitude', 'v', 'altitude', 'azimuth', 'frac')})
    ms, _ = E.timed(lambda: R.source_map(outs, few.unit_km, None, 'source', True, 1.0))
    return dict(restatement_source_only_ms=round(ms, 1))


if __name__ == '__main__':
    E.main([float(a) for a in sys.argv[1:]] or None, extra=restatement_ms)
