"""Worker of tests/test_gpu_pillar_exact.py::test_knobs_read_once_per_process: the pillar library reads LAV_PILLAR_ZERO, LAV_PILLAR_REC
and LAV_PILLAR_WG_PER_CU once per process, so each setting runs in a process of its own.  Runs the class X cases of
tests/pillar_exact_util.py's KNOB_CASES (and KNOB_EXTRA: point width 8 and the VALU build, which the same knobs rebuild too) through
ops.pillar_scatter and writes canvases and indices to OUT_DIR/out.npz; the parent compares them with float64.

    python tests/_pillar_knob_worker.py OUT_DIR
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np   # noqa: E402
import torch         # noqa: E402


def main():
    from lav_amd import ops
    from tests import pillar_exact_util as P
    dev = torch.device("cuda")
    out = {}
    for grid, D, kind, impl in [c + ("mfma",) for c in P.KNOB_CASES] + P.KNOB_EXTRA:
        case = P.x_case(grid, D, kind)
        os.environ["LAV_PILLAR_IMPL"] = impl
        w = [torch.from_numpy(a).to(dev) for a in (case.w1, case.b1, case.w2, case.b2)]
        canvas, uc, inv = ops.pillar_scatter(torch.from_numpy(case.points).to(dev), case.n, ops.make_grid(*case.grid.args), *w, want_indices=True)
        key = f"{grid}/{D}/{kind}/{impl}"
        out[key + "/canvas"], out[key + "/uc"], out[key + "/inv"] = canvas.cpu().numpy(), uc.cpu().numpy(), inv.cpu().numpy()
    torch.cuda.synchronize()
    np.savez_compressed(os.path.join(sys.argv[1], "out.npz"), **out)


if __name__ == "__main__":
    main()
