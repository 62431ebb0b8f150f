"""The one-process-per-GPU path on the real library (sorts last on purpose: these tests spawn torch.distributed
jobs, and a failure here must not hide the parity suites from a `pytest -x` run).

A 1-GPU box stands in for N GPUs: every rank opens its own context on device 0 (RT_BENCH_ONE_DEVICE=1) and the
collective runs over gloo (RCCL refuses two ranks on one device) — the partition, the bound render targets, the
gather and bench.py's own N > 1 bookkeeping are the code the driver's SCALE run executes."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_NET_ERRORS = ("ddress already in use", "EADDRINUSE", "DistNetworkError", "RendezvousConnectionError", "Connection reset by peer", "Socket Timeout",
               "failed to bind", "connectFullMesh")


def _run_retrying_rendezvous(make_cmd, env, timeout):
    """Run a torch.distributed job; ONE retry on a fresh port if — and only if — it died of a rendezvous / socket error (the port
    _free_port() hands out can be taken by a closing socket of the previous job before the launcher binds it: seen once in 130 runs on
    the GPU box, round 6).  A numerical mismatch or any other failure is never retried."""
    p = None
    for attempt in range(2):
        p = subprocess.run(make_cmd(), capture_output=True, text=True, timeout=timeout, env=env)
        if p.returncode == 0 or not any(e in p.stderr for e in _NET_ERRORS) or "AssertionError" in p.stderr:
            break
    return p


def _report(p):
    """Head AND tail of both streams: the first failing rank's traceback is usually not in the last 4 KB."""
    def cut(t):
        return t if len(t) <= 12000 else t[:6000] + "\n...[cut]...\n" + t[-6000:]
    tagged = "\n".join(l for l in p.stderr.splitlines() if l.startswith("[rank "))
    return f"rc={p.returncode}\n--- rank-tagged failures\n{tagged}\n--- stdout\n{cut(p.stdout)}\n--- stderr\n{cut(p.stderr)}"


@pytest.mark.gpu
@pytest.mark.parametrize("world,cfg", [(2, 3), (3, 2)])
def test_partitioned_contexts_bound_targets_and_gather_on_the_gpu(world, cfg):
    """rt_set_partition + rt_bind_render_targets + the gather, together, on the real library (one device,
    `world` processes, gloo for the collective) == the oracle's single image."""
    def cmd():
        return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_dist_worker.py"), "gpu", str(cfg)]
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = _run_retrying_rendezvous(cmd, env, 900)
    assert p.returncode == 0, _report(p)
    assert "DIST_GPU_OK" in p.stdout


def _bench_run(world, *extra, one_device=True, env_extra=None):
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(env_extra or {})
    if one_device:
        env.update(RT_BENCH_ONE_DEVICE="1", RT_BENCH_BACKEND="gloo")
    else:
        env.pop("RT_BENCH_ONE_DEVICE", None)
        env.pop("RT_BENCH_BACKEND", None)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return _run_retrying_rendezvous(lambda: [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--no-cpu-baseline", "--no-pmc", *extra], env, 1500)


def _bench(world, *extra, one_device=True, env_extra=None):
    p = _bench_run(world, *extra, one_device=one_device, env_extra=env_extra)
    assert p.returncode == 0, _report(p)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, _report(p)
    return json.loads(lines[0])


def _check_multi_rank_line(d, world, steps, resolution, distinct=1):
    assert d["n_gpus"] == world and d["steps"] == steps and d["resolution"] == resolution
    assert d["value"] > 0 and d["gather_ms"] is not None and d["gather_error"] is None
    # every rank took part and said which device it ran on (one shared device here: the test hook)
    assert d["ranks_seen"] == world
    assert sorted(r["rank"] for r in d["devices_seen"]) == list(range(world))
    assert len({r["pid"] for r in d["devices_seen"]}) == world
    assert d["distinct_devices"] == distinct
    # the gathered image holds every frame of every rank's strips ...
    assert d["gathered_image_complete"] is True, d["gathered_image"]
    assert d["gathered_image"]["alpha_min"] == d["gathered_image"]["alpha_max"] == d["gathered_image"]["alpha_expected"]
    # ... and equals the oracle's on strips owned by every rank
    par = d["gathered_image"]["parity_vs_oracle"]
    assert par["bit_identical"] is True and par["rel_l2_per_channel"] == [0.0, 0.0, 0.0], par
    assert par["ranks_covered"] == list(range(world))
    assert d["diagnostics"] == []


@pytest.mark.gpu
def test_bench_spawns_its_own_ranks():
    """`python bench.py --gpus 2` with WORLD_SIZE unset starts the two ranks itself (strong scaling on the
    BASELINE image); the line it prints proves both ranks rendered and that the gathered image is the oracle's."""
    d = _bench(2, "--steps", "3", "--warmup", "1")
    assert d["scaling"] == "strong"
    _check_multi_rank_line(d, 2, 3, [1920, 1080])


@pytest.mark.gpu
def test_bench_ranks_stay_on_the_same_frames_under_skew():
    """round 5's wall-clock-bounded spin-up let ranks render different numbers of untimed frames (48 vs 52 on the
    driver's box), so they timed different Frame indices and the gathered image mixed frame sets.  Nothing in bench.py may depend on a
    rank's own clock: odd ranks are held back 25 ms before every pass (RT_BENCH_RANK_SKEW_MS) and the line must still prove that every
    rank rendered the same frames — alpha == frames everywhere, first timed Frame = W + 1, the regions' steps equal on all ranks."""
    d = _bench(2, "--steps", "3", "--warmup", "2", "--regions", "3", "--region-ms", "8", env_extra={"RT_BENCH_RANK_SKEW_MS": "25"})
    _check_multi_rank_line(d, 2, 3, [1920, 1080])
    assert d["config"]["first_timed_frame"] == 3 and "spinup" not in d
    g = d["regions"]
    assert g["n"] == 3 and g["steps_each"] >= 3 and g["first_frame"] == 3 + 3 and len(g["values"]) == 3 and min(g["values"]) > 0
    # every frame of every pass is in the gathered image: W + K + regions + RenderFrame pass + stats replay + batched replay
    assert d["gathered_image"]["alpha_expected"] == 2 + 3 + 3 * g["steps_each"] + 3 * 3


@pytest.mark.gpu
def test_bench_four_ranks_on_the_north_star_workload():
    """BASELINE.json configs[4] as the driver's multi-GPU run executes it (3840x2160, 12 bounces, 983k triangles, image
    row-tiled over the ranks), reduced to 2 steps, the ranks sharing this box's GPU.  Four ranks: with this test process, five
    processes hold the GPU at once, under the six a shared GPU may have open."""
    d = _bench(4, "--config", "5", "--steps", "2", "--warmup", "1", "--no-batched", "--regions", "1", "--region-ms", "1")
    _check_multi_rank_line(d, 4, 2, [3840, 2160])


def _gpu_count():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


@pytest.mark.gpu
def test_bench_two_gpus_over_rccl():
    """The path the driver's SCALE run takes, on real hardware when the box has it: one rank per GPU, backend "nccl" (= RCCL over
    xGMI), the gather between DISTINCT devices; gathered image == the oracle's, two distinct devices reported.  A box with one GPU
    cannot give the ranks distinct devices: there the same command must refuse on every rank, before any rank selects a device it
    does not have or waits in the process group's set-up, and print no line."""
    n = _gpu_count()
    assert n >= 1
    if n < 2:
        p = _bench_run(2, "--steps", "3", "--warmup", "1", one_device=False)
        assert p.returncode != 0, _report(p)
        assert f"bench.py: 2 ranks on this node need 2 GPUs, {n} visible" in p.stderr, _report(p)
        # the refusal, not a rank failing on a device it does not have (run() tags such failures "[rank r] bench.py failed")
        assert "bench.py failed" not in p.stderr and "invalid device ordinal" not in p.stderr, _report(p)
        assert not any(l.startswith("{") for l in p.stdout.splitlines()), _report(p)
        return
    d = _bench(2, "--steps", "3", "--warmup", "1", one_device=False)
    _check_multi_rank_line(d, 2, 3, [1920, 1080], distinct=2)
    assert all(r["backend"] == "nccl" for r in d["devices_seen"])


@pytest.mark.gpu
def test_bench_one_rank_through_rccl():
    """Everything the driver's SCALE run does that a 1-GPU box can execute, on backend "nccl" (= RCCL): a ONE-rank job forced down
    the distributed path (RT_BENCH_FORCE_DIST=1) — init_process_group("nccl", device_id=...), the NUMA pinning, partition 1/1 with
    bound render targets, dist.gather of device tensors + the de-interleave, all_reduce on device tensors, all_gather_object,
    barrier, destroy — and the gathered image equals the oracle's."""
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", RT_BENCH_FORCE_DIST="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RT_BENCH_ONE_DEVICE", "RT_BENCH_BACKEND", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-cpu-baseline", "--no-pmc", "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, _report(p)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, _report(p)
    d = json.loads(lines[0])
    _check_multi_rank_line(d, 1, 3, [1920, 1080])
    assert d["devices_seen"][0]["backend"] == "nccl"


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,w,h", [(2, 200, 77), (3, 96, 54)])
def test_gather_over_a_caller_owned_rccl_communicator(pkg, api, orc, cfg, w, h):
    """rt_gather_rccl (the C ABI's own RCCL gather, no torch): a one-rank communicator made with librccl's ncclCommInitAll, the
    context partitioned 1/1 — ncclGroupStart, a send and a receive of the packed tile, ncclGroupEnd, the de-interleave kernel —
    and the gathered image equals the context's own read-back and the oracle's image.  Wrong communicators are refused."""
    import ctypes as C
    import numpy as np
    import torch
    rccl = C.CDLL("librccl.so.1")
    comm = C.c_void_p()
    dev = (C.c_int * 1)(0)
    torch.cuda.set_device(0)
    assert rccl.ncclCommInitAll(C.byref(comm), 1, dev) == 0
    try:
        tr = api.create_tracer(0)
        tr.set_partition(8, 0, 1)
        mgr = pkg.scenes.get(cfg).make_manager(tr, api, w, h)
        mgr.OnEnable(renderSeed=5)
        mgr.RenderFrames(3)
        out = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda:0")
        tr.gather_rccl(comm, 0, out.data_ptr(), out.numel() * 4, accumulated=True)
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), tr.read_accumulated().view(np.uint32))
        frame = torch.empty_like(out)
        tr.gather_rccl(comm, 0, frame.data_ptr(), frame.numel() * 4, accumulated=False)
        assert np.array_equal(frame.cpu().numpy().view(np.uint32), tr.read_frame().view(np.uint32))
        ref = orc.create_tracer(8)
        m2 = pkg.scenes.get(cfg).make_manager(ref, orc, w, h)
        m2.OnEnable(renderSeed=5)
        m2.RenderFrames(3)
        assert np.array_equal(got.view(np.uint32), ref.read_accumulated().view(np.uint32))
        ref.close()
        # the communicator's rank / size must be the context's partition
        tr2 = api.create_tracer(0)
        tr2.set_partition(8, 0, 2)
        tr2.resize(w, h)
        with pytest.raises(pkg.abi.RtError):
            tr2.gather_rccl(comm, 0, out.data_ptr(), out.numel() * 4)
        tr2.close()
        with pytest.raises(pkg.abi.RtError):
            tr.gather_rccl(comm, 0, out.data_ptr(), 16)        # wrong size
        with pytest.raises(pkg.abi.RtError):
            tr.gather_rccl(None, 0, out.data_ptr(), out.numel() * 4)
        tr.close()
    finally:
        rccl.ncclCommDestroy(comm)


@pytest.mark.gpu
def test_multi_context_peer_access_is_reported(pkg, api):
    """rt_create_multi checks / enables peer access between its distinct devices and says how device-to-device copies travel."""
    import ctypes as C
    n = _gpu_count()
    ids = (C.c_int * 2)(0, 1 if n >= 2 else 0)
    m = C.c_void_p()
    assert api.create_multi(ids, 2, C.byref(m)) == 0
    pairs, enabled = C.c_int(-1), C.c_int(-1)
    rc = api.multi_peer_access(m, C.byref(pairs), C.byref(enabled))
    if n >= 2:
        assert pairs.value == 2 and rc in (0, 1, 2) and 0 <= enabled.value <= 2
    else:
        assert rc == -1 and pairs.value == 0 and enabled.value == 0  # the same device twice: nothing to copy between devices
    api.destroy_multi(m)
