"""The forest builder's kNN on a list of cases of tests/forest_shapes_ref.py, in a process of
its own: PQH_KNN_IMPL and PQH_KNN_SELECT are read once per process, so only a fresh child can
run the all-VALU kernel or the lane-per-query selection.  tests/test_gpu_forest_shapes.py sets
the variable, starts this file once per variant and compares what it wrote with the oracle.

    python knn_worker.py CASES.json OUTDIR

CASES.json is a list of case names; OUTDIR gets one <name>.npz each (starts, ends, idx as
uint32, dist, sizes).  The first error ends the run with a non-zero status."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def run_case(torch, forest, ctx, c):
    """(starts, ends, idx uint32, dist, sizes) of one case; a padded case goes in as a view of
    a wider tensor whose extra columns are NaN"""
    x = c["x"]
    if c["pad"]:
        big = np.full((x.shape[0], x.shape[1] + c["pad"]), np.nan, np.float32)
        big[:, :x.shape[1]] = x
        xd = torch.from_numpy(big).cuda()[:, :x.shape[1]]
        assert xd.stride(0) == big.shape[1]
    else:
        xd = torch.from_numpy(np.array(x)).cuda()
    st, en = forest.blocks_info(ctx, xd, c["ns"], c["nb"], c["ov"])
    idx, dist, sizes = forest.knn_fast(ctx, xd, c["nn"], *(c["geo"] or (st, en)))
    torch.cuda.synchronize()
    return st, en, idx, dist, sizes


def main():
    names = json.load(open(sys.argv[1]))
    out = sys.argv[2]
    import torch
    import forest_shapes_ref as fs
    from pq_huffman_amd import codec, forest
    ctx = codec.Context(0)
    for name in names:
        st, en, idx, dist, sizes = run_case(torch, forest, ctx, fs.build(name))
        np.savez(os.path.join(out, name + ".npz"), starts=st, ends=en,
                 idx=idx.cpu().numpy().view(np.uint32), dist=dist.cpu().numpy(), sizes=sizes)
    ctx.close()
    print(f"knn_worker: {len(names)} cases, PQH_KNN_IMPL={os.environ.get('PQH_KNN_IMPL')} "
          f"PQH_KNN_SELECT={os.environ.get('PQH_KNN_SELECT')}")


if __name__ == "__main__":
    main()
