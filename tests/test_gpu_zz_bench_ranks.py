"""bench.py itself, run as a child process, against the oracle: the multi-rank schedule on one
GPU (gloo process group, every rank on cuda:0) -- the library's two-phase pqh_shard_encode, or
the Python composition (halo all-gather, histogram all-reduce, device bit offsets,
encode_write_at) -- whose shards' streams stitched on rank 0 must equal the oracle's one-shot
stream over all ranks' rows (huffman_encoder.c:207-238 over the concatenated input); the
multi-rank pipeline over RCCL with one rank; and the one-rank headline schedule itself.  Every
run dumps its rows and centroids, so the codes are checked against the oracle's assignment
too, and every rank must exit cleanly (status 0, no signal at teardown)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, run_fail_msg

pytestmark = pytest.mark.gpu


# torchrun's own c10d store binds port 0 and the ranks reuse it (TORCHELASTIC_USE_AGENT_STORE):
# no port is picked here and released before the launcher binds it.
_LAUNCH = ["--standalone", "--local-addr=127.0.0.1"]


def _check_assignment(oracle, d):
    """the ranks' part-major assignment (pqh_pq_assign_parts, the bench's timed kernel) equals
    the oracle's fp32 first-minimum assignment of the same rows (src/pq_encoder.c:270-272)"""
    want, _ = oracle.pq_assign(d["x"], d["cent"], threads=0)
    bad = int((d["codes"] != want).sum())
    assert bad == 0, f"{bad} PQ codes differ from the oracle"


@pytest.mark.parametrize("path", ["library", "python"])
@pytest.mark.parametrize("mode", ["ctx", "noctx"])
def test_two_rank_rehearsal_stitched_stream(oracle, tmp_path, mode, path):
    """path library: the bench's default world > 1 schedule through the C ABI
    (pqh_shard_encode_tables on the table lane, pqh_shard_encode_write on the encode stream,
    torch.distributed hooks); python: the same steps composed in shard.py."""
    dump = tmp_path / "dump.npz"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           *_LAUNCH,
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
           "--one-device", "--vectors", "30001", "--steps", "3", "--warmup", "1",
           "--mode", mode, "--full", "--no-cpu-baseline", "--dump", str(dump),
           "--shard-path", path]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, run_fail_msg(r)
    d = np.load(dump, allow_pickle=False)
    codes = d["codes"]
    assert codes.shape == (60002, 8)
    _check_assignment(oracle, d)
    cbs = oracle.build_codebooks(codes, 256, mode == "ctx")
    want, bits = oracle.encode(codes, cbs)
    assert int(d["bits"]) == bits
    assert d["stream"].tobytes() == want


@pytest.mark.parametrize("groups", ["one", "lanes"])
def test_one_rank_rccl_rehearsal_stream(oracle, tmp_path, groups):
    """bench.py --dist-rehearse: the world > 1 pipeline (process group over RCCL, the
    TorchComm hooks, both pqh_shard_encode phases, stream A on its own hardware queue) with
    one rank -- the nccl route on hardware; the rank's stream must equal the oracle's and
    the bench's own checks (round trip, row-path re-encode, shard status) must pass."""
    dump = tmp_path / "dump.npz"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           *_LAUNCH,
           os.path.join(ROOT, "bench.py"), "--dist-rehearse", "--shard-groups", groups,
           "--vectors", "30001", "--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline",
           "--dump", str(dump)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, run_fail_msg(r)
    d = np.load(dump, allow_pickle=False)
    codes = d["codes"]
    assert codes.shape == (30001, 8)
    _check_assignment(oracle, d)
    cbs = oracle.build_codebooks(codes, 256, True)
    want, bits = oracle.encode(codes, cbs)
    assert int(d["bits"]) == bits
    assert d["stream"].tobytes() == want


@pytest.mark.parametrize("config,mode", [("sift", "ctx"), ("deep", "ctx"), ("sift", "noctx")])
def test_one_rank_bench_stream(oracle, tmp_path, config, mode):
    """bench.py exactly as the headline runs it at one rank (no process group: stream A's
    part-major assignment, the histogram and code tables on the table lanes, the part-major
    encoder and the decoder on the encode stream, 4-vector chunks), on a small batch: its last
    batch's codes equal the oracle's assignment and its stream the oracle's encoding of them
    (src/pq_encoder.c:270-272, src/huffman_encoder.c:207-238)."""
    dump = tmp_path / "dump.npz"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--mode", mode,
           "--vectors", "30001", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
           "--device-warmup-ms", "0", "--dump", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, run_fail_msg(r)
    d = np.load(dump, allow_pickle=False)
    codes = d["codes"]
    assert codes.shape == (30001, 16 if config == "deep" else 8)
    _check_assignment(oracle, d)
    cbs = oracle.build_codebooks(codes, 256, mode == "ctx")
    want, bits = oracle.encode(codes, cbs)
    assert int(d["bits"]) == bits
    assert d["stream"].tobytes() == want


def test_plain_bench_dump_outputs(oracle, tmp_path):
    """a plain run (no --full): the line carries the headline fields for `--steps` timed steps
    and none of --full's figures, and --dump-outputs writes the last timed step's arrays as
    float32 / float64 .npy, at most 64 MB in all: at this size every row, byte and chunk, so
    the codes equal the oracle's assignment, `decoded` the codes, the stream and its length
    the oracle's encoding, and the chunk index each chunk's previous row."""
    import json
    dump, outs = tmp_path / "dump.npz", tmp_path / "outs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--vectors", "30001",
           "--steps", "3", "--warmup", "1", "--device-warmup-ms", "0", "--dump", str(dump),
           "--dump-outputs", str(outs)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, run_fail_msg(r)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "Mvec/s"
    # value = vectors / step time (both rounded in the line: 3 and 2 decimals)
    rel = 0.0006 / line["ms_per_step"] + 0.006 / line["value"]
    assert abs(line["value"] * line["ms_per_step"] * 1e3 / 30001 - 1) <= rel
    for key in ("metric", "higher_is_better", "dtype"):
        assert key in line
    for key in ("cpu_baseline", "pcie_ms", "stages_ms"):
        assert key not in line
    a = {f[:-4]: np.load(outs / f, allow_pickle=False) for f in sorted(os.listdir(outs))}
    assert set(a) == {"codes", "decoded", "stream", "stream_bits", "chunk_offsets", "chunk_prev"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    d = np.load(dump, allow_pickle=False)
    want, _ = oracle.pq_assign(d["x"], d["cent"], threads=0)
    assert np.array_equal(a["codes"], want) and np.array_equal(a["decoded"], want)
    stream, bits = oracle.encode(want, oracle.build_codebooks(want, 256, True))
    assert int(a["stream_bits"][0]) == bits
    assert a["stream"].astype(np.uint8).tobytes() == stream[:(bits + 7) // 8]
    assert a["chunk_offsets"].shape == ((30001 + 3) // 4,) and a["chunk_offsets"][0] == 0
    assert np.all(np.diff(a["chunk_offsets"]) > 0) and a["chunk_offsets"][-1] < bits
    assert np.array_equal(a["chunk_prev"][1:], want[3:-1:4])
