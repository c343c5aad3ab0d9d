"""Real multi-GPU execution of the N > 1 paths.  Every test here skips unless >= 2 devices are visible (the round's test box has
one); on a multi-GPU node they are the first contact of the RCCL code with hardware:

  * the torch.distributed path bench.py uses under the driver's launch (tiling.exchange_halo / allgather_slabs, backend nccl = RCCL):
    two ranks on two GPUs render the hybrid frame's bands and compare them with the un-tiled render (tools/frame_bench.py --check);
  * the native transport a C++ host links (libhr_comm.so: hr_comm_create_rccl, grouped ncclSend / ncclRecv, tickets):
    tools/native_comm_check.py under the same launch, and examples/tiled_frame (threads, one per GPU);
  * bench.py --gpus 2: the line carries comm.ranks_seen == 2 and the hybrid_4k block with its communication times.
The same code runs on ONE GPU through gloo (tests/test_gpu_tiling.py, tests/test_tiling_gloo.py) and the loopback transport
(tests/test_gpu_comm.py)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n_devices():
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def _launch(script_args, n=2, timeout=900, env=None):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(port)] + script_args
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    e.update(env or {})
    out = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(lines[-1]), out


needs_two = pytest.mark.skipif(_n_devices() < 2, reason="needs >= 2 GPUs (RCCL refuses two ranks on one device)")


@needs_two
def test_two_gpus_torch_distributed_rccl_bands_equal_untiled():
    j, out = _launch([os.path.join(ROOT, "tools", "frame_bench.py"), "--gpus", "2", "--width", "960", "--height", "544", "--frames", "2", "--warmup", "1",
                      "--detail", "0.25", "--probes", "6,3,4", "--rays-per-probe", "64", "--check"])
    assert j["n_gpus"] == 2 and j["bit_identical_to_untiled"] is True, (j, out.stderr[-2000:])


@needs_two
def test_two_gpus_native_rccl_transport():
    j, out = _launch([os.path.join(ROOT, "tools", "native_comm_check.py")])
    assert j["ranks_seen"] == 2 and j["bit_identical_to_untiled"] is True and j["last_ticket"] > 0, (j, out.stderr[-2000:])


@needs_two
def test_cpp_tiled_frame_uses_rccl_with_two_devices():
    exe = os.path.join(ROOT, "examples", "_build", "tiled_frame")
    if not os.path.exists(exe):
        pytest.skip("examples/_build/tiled_frame not built (run __graft_entry__.build())")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0 and "transport RCCL" in out.stdout and "every band row equals the un-tiled render" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@needs_two
def test_bench_two_gpus_reports_ranks_and_comm_times():
    j, out = _launch([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--full"], timeout=1500)
    assert j["n_gpus"] == 2 and j["comm"]["ranks_seen"] == 2 and j["comm"]["backend"] == "nccl", j.get("comm")
    assert j["comm"]["exchange_us_per_frame"] > 0 and len(j["comm"]["band_bounds"]) == 3
    assert "passes_error" not in j, j["passes_error"]
    h = j["hybrid_4k"]
    assert h["n_gpus"] == 2 and h["comm_us_per_frame"]["ddgi_atlas_allgather"] > 0 and h["ms_per_frame"] > 0


def test_bench_two_ranks_on_one_gpu_gloo():
    """the N > 1 code path of bench.py on the one GPU of the test box (gloo, both ranks on device 0): functional check of the line's
    `comm` block and of the hybrid_4k block — what the driver's --gpus N launch executes with RCCL"""
    if _n_devices() < 1:
        pytest.skip("no GPU")
    j, out = _launch([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2", "--full", "--no-cpu-baseline"], timeout=1500,
                     env=dict(HR_DIST_BACKEND="gloo", HR_FORCE_DEVICE="0"))
    assert j["n_gpus"] == 2 and j["comm"]["ranks_seen"] == 2 and j["comm"]["backend"] == "gloo"
    assert len(j["comm"]["band_bounds"]) == 3 and j["comm"]["exchange_us_per_frame"] > 0
    assert "passes_error" not in j, j["passes_error"]
    assert j["hybrid_4k"]["n_gpus"] == 2 and set(j["hybrid_4k"]["comm_us_per_frame"]) >= {"shadows_exchange", "ao_exchange", "reflections_exchange", "ddgi_atlas_allgather"}
    assert j["hybrid_4k"]["forked_streams"] is False and j["timed_repeats"] >= 1


def test_bench_two_ranks_forked_hybrid_frame_gloo():
    """HR_FRAME_FORKED=1: the N > 1 hybrid frame with its three chains on three torch streams (frame.py _render_forked) — must run (no
    fall-back to the serial frame) and give the same ray counts as the serial one"""
    if _n_devices() < 1:
        pytest.skip("no GPU")
    args = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline"]
    jf, _ = _launch(args, timeout=1500, env=dict(HR_DIST_BACKEND="gloo", HR_FORCE_DEVICE="0", HR_FRAME_FORKED="1"))
    assert "passes_error" not in jf, jf["passes_error"]
    assert jf["hybrid_4k"]["forked_streams"] is True and "forked_error" not in jf["hybrid_4k"], jf["hybrid_4k"]
    assert jf["hybrid_4k"]["ms_per_frame"] > 0 and jf["hybrid_4k"]["Mrays_per_s"] > 0
