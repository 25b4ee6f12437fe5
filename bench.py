#!/usr/bin/env python3
"""Headline benchmark: SSGD logistic regression, samples/sec (whole node).

BASELINE.json metric "samples/sec (whole node) SSGD logistic regression at
1/2/4/8 MI355X", config "SSGD logistic regression 10M x 1024 bf16": a global
10M-row x 1024-feature bf16 dataset (synthetic, generated on device from a planted
logistic model) is row-sharded over the N ranks (strong scaling: the global
problem is fixed, each GPU holds N_rows/N rows in HBM). One step = the
reference's SSGD iteration (optimization/ssgd.py:93-105): Bernoulli(0.1)
minibatch + fused gradient (K1+K7) -> RCCL all_reduce([g || count]) -> K8 update,
every rank. samples/sec = global minibatch rows processed per second (exact
count, accumulated on device).

Run: python bench.py [--gpus N --steps K --warmup W]. With N > 1 and no launcher
environment the script starts ``torch.distributed.run --nproc-per-node N`` on itself
as a CHILD process (before anything touches the GPU; no exec) and exits with its
code, so one command measures N ranks on N GPUs (RCCL over xGMI); under
torchrun (the driver's N > 1 launch) it is one of the ranks. The JSON carries the
evidence that N distinct devices took part (``device_ids``), the RCCL version and
the small-all-reduce path the start-up race chose with both timings.

A plain run does only what the headline figure needs: data generation, warmup, the
launch-form calibration (it decides which form the timed steps run), the K timed steps,
the result line. ``--dump-outputs DIR`` also writes what the timed steps computed (the
model after the last timed step, the exact sampled-row count) as ``DIR/<name>.npy``; the
inputs are seeded, so two builds can be compared output for output.

``--full`` adds everything else, after the timed region and untimed by it: the per-step
all-reduce time measured in isolation, the held-out accuracy of the trained model (a
correctness witness: a fast but wrong gradient kernel fails the run), and, at every N on
GPUs (``--secondary``), BASELINE configs #3-#5 under a ``secondary`` key of the same JSON
line: BMUF and EASGD on the headline's data (exact sampled-row counts, held-out
witnesses), the k-means reference job at 100M x 128, k = 1024 (also on overlapping
clusters) and the PageRank reference job at R-MAT scale 26 (adjacency build + 10
iterations), each with its witness (dalgo/apps/jobs.py). A failed witness, headline or
secondary, makes the exit code non-zero.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

BASELINE_METRIC = "samples/sec (whole node) SSGD logistic regression at 1/2/4/8 MI355X"
BASELINE_VALUE = None   # the reference publishes no throughput numbers


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--frac", type=float, default=0.1)
    ap.add_argument("--algo", default="ssgd", choices=["ssgd", "gd", "ma", "bmuf", "easgd"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--backend", default=None, choices=["nccl", "gloo"],
                    help="collective backend (default: nccl = RCCL on GPU, gloo on CPU)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run what the headline figure does not "
                         "need: the all-reduce probe, the held-out witness (--eval) and the "
                         "secondary configs (--secondary); without it those options are idle")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed steps computed (model after the last timed "
                         "step, sampled-row count) as DIR/<name>.npy")
    ap.add_argument("--eval", dest="eval", action="store_true", default=True,
                    help="with --full: held-out accuracy after the timed region (default on)")
    ap.add_argument("--no-eval", dest="eval", action="store_false")
    ap.add_argument("--n-test", type=int, default=100_000, help="held-out rows for the witness")
    ap.add_argument("--witness-steps", type=int, default=1500,
                    help="after the timed region, keep training (untimed) up to this many total "
                         "steps (the reference's n_iterations, optimization/ssgd.py:18) before "
                         "the held-out evaluation")
    ap.add_argument("--launch", default=os.environ.get("DALGO_LAUNCH", "auto"),
                    choices=["auto", "env"],
                    help="auto: time the equivalent SSGD/GD step launch forms (per-step K1 + "
                         "update/K11, one fused launch per step, one persistent launch per K "
                         "steps) after the warmup, untimed, and keep the fastest; env: the "
                         "DALGO_ONE_KERNEL / DALGO_PERSISTENT settings")
    ap.add_argument("--cal-steps", type=int, default=20, help="steps per candidate (auto)")
    ap.add_argument("--cal-budget-s", type=float, default=20.0,
                    help="wall-clock budget of the launch calibration (auto): no further "
                         "candidate form is raced once it is spent")
    ap.add_argument("--pg-timeout-s", type=float, default=120.0,
                    help="process-group timeout: an RCCL collective stuck longer aborts the rank")
    ap.add_argument("--secondary", default="auto", choices=["auto", "on", "off"],
                    help="with --full: after the headline, the BMUF / EASGD, k-means and PageRank jobs "
                         "(BASELINE configs #3-#5) under a 'secondary' key of the same JSON "
                         "line, at every N; auto = on for GPU runs")
    ap.add_argument("--secondary-budget-s", type=float, default=240.0,
                    help="no further secondary config starts once this much wall clock is spent")
    ap.add_argument("--secondary-steps", type=int, default=20)
    ap.add_argument("--secondary-warmup", type=int, default=5)
    ap.add_argument("--km-rows", type=int, default=100_000_000)
    ap.add_argument("--km-hard-noise", type=float, default=4.0,
                    help="blob noise of the overlapping-cluster k-means run")
    ap.add_argument("--pr-scale", type=int, default=26)
    ap.add_argument("--km-pool-gb", type=float, default=48.0,
                    help="device memory the k-means job's caching allocator holds (per rank; "
                         "divided among ranks that share one GPU)")
    ap.add_argument("--pr-pool-gb", type=float, default=96.0,
                    help="the same for the PageRank job")
    ap.add_argument("--deadline-s", type=float, default=540.0,
                    help="wall-clock deadline per rank: past it the rank prints its stacks and "
                         "exits 124 (a hang becomes a fast, rank-tagged failure); 0 = off")
    a = ap.parse_args(argv)
    if not a.full:   # a plain run: the headline alone
        a.eval, a.secondary = False, "off"
    return a


def calibrate_launch(model, rt, a) -> dict:
    """Pick the fastest launch form of the SAME training step on this node.

    The three forms compute identical steps (tests/test_gpu_multirank.py::
    test_fused_xgmi_update_matches_process_group); which one is fastest depends on the
    node (launch latency vs. the xGMI exchange latency the persistent form hides under
    the next step's first row loads), so it is measured rather than assumed. Runs after
    the warmup and before the timed region (untimed); every rank times every candidate,
    the MAX over ranks decides, so all ranks pick the same form. Returns the per-candidate
    ms/step."""
    from dalgo.parallel import comm, runtime
    if (a.algo not in ("ssgd", "gd") or model.device.type != "cuda" or not model._zg
            or model._graph_ok() or a.cal_steps <= 0):
        return {}
    if comm.world_size() > 1 and model.bucket.xg is None:
        return {}   # the fused / persistent forms need the K11 exchange on several ranks
    # ranks sharing one GPU (the one-GPU rehearsals): a rank's in-kernel wait for its peers'
    # exchange needs the peers' kernels co-resident on the same CUs, which a persistent grid
    # does not leave room for; the forms are only raced when every rank has its own GPU
    # (library rule, from the device identities every rank published at init)
    if not runtime.spin_waits_allowed():
        return {}
    # the calibration trains extra steps: restore the model afterwards so the timed region
    # and the held-out witness see exactly warmup + steps training steps
    snap = model.state_dict()
    # per-step first (no kernel waits on another GPU); the forms whose kernels spin on a
    # peer (one-kernel / persistent release across ranks) only while every earlier form
    # came back clean (collective device-error check after each) and the calibration
    # stays inside its wall-clock budget (decided on the MAX-over-ranks clock, so every
    # rank stops at the same candidate). On several ranks they also need the K11 exchange,
    # which exists only if its collective self-test AND the start-up race passed.
    # "graph": the per-step kernels (K1 + K11 exchange/update) replayed from one captured
    # hipGraph -- the K11 epoch is device-resident, so the capture is replay-safe
    cands = {"per-step": (False, False, False), "graph": (False, False, True),
             "one-kernel": (True, False, False), "persistent": (False, True, False)}
    res = {}
    spent = 0.0
    for name, (one, pers, graph) in cands.items():
        if name != "per-step" and spent > a.cal_budget_s:
            res["stopped"] = f"budget {a.cal_budget_s:.0f} s spent before {name}"
            break
        model._ok1, model._okp = one, pers
        model.graph, model._okg = graph, None
        t_all = time.perf_counter()
        # first launch of this form (code objects, workspaces; graph: warm step + capture).
        # A form that raises on any rank is dropped on every rank (MAX of a failure flag)
        bad = torch.zeros(1, dtype=torch.float64, device=rt.device)
        try:
            model.run_steps(2)
            rt.synchronize()
        except Exception as e:   # noqa: BLE001 -- reported, then decided collectively
            print(f"[bench] rank {rt.rank}: launch form {name} failed: {e!r}", file=sys.stderr,
                  flush=True)
            bad.fill_(1.0)
        comm.all_reduce_max(bad)
        if float(bad.item()) > 0:
            res[name] = None              # dropped on every rank
            model.graph, model._okg = False, None
            model._graphs.clear()
            model._ok1, model._okp = False, False
            # a form that raised after K1 ran can leave partial sums in [g || count]:
            # clear it, and tell the next gradient launch the bucket is not known zero
            if hasattr(model, "bucket"):
                model.bucket.buffer.zero_()
            model._g_zero = False
            try:
                comm.check_device_errors(f"launch calibration ({name})")
            except comm.DeviceCollectiveError:
                fallback_plain(model, rt, f"launch calibration ({name})")
                model.load_state_dict(snap)
                rt.synchronize()
                return {"failed": name, **res}
            model.load_state_dict(snap)
            continue
        rt.barrier()
        rt.synchronize()
        t0 = time.perf_counter()
        model.run_steps(a.cal_steps)
        rt.synchronize()
        rt.barrier()
        rt.synchronize()
        el = torch.tensor([time.perf_counter() - t0, time.perf_counter() - t_all],
                          dtype=torch.float64, device=rt.device)
        comm.all_reduce_max(el)
        res[name] = float(el[0].item()) / a.cal_steps * 1e3
        spent += float(el[1].item())
        try:
            comm.check_device_errors(f"launch calibration ({name})")
        except comm.DeviceCollectiveError:
            fallback_plain(model, rt, f"launch calibration ({name})")
            model.load_state_dict(snap)
            rt.synchronize()
            return {"failed": name, **res}
    timed = {k: v for k, v in res.items() if k in cands and v is not None}
    if not timed:   # every form raised: keep the plain per-step form
        fallback_plain(model, rt, "launch calibration (no form ran)")
        model.load_state_dict(snap)
        rt.synchronize()
        return {"failed": "all", **res}
    best = min(timed, key=timed.get)
    model._ok1, model._okp, graph = cands[best]
    model.graph, model._okg = graph, None
    model.load_state_dict(snap)
    rt.synchronize()
    return res


def fallback_plain(model, rt, why: str) -> None:
    """A device-side wait (K11 peer flag, persistent step release) timed out on some rank
    (collective check raised everywhere): switch EVERY rank to the plain per-step form
    over the process group -- no kernel waits on another GPU any more -- and clear the
    error words. The caller restores the model and measures again.

    A launch that stopped early can leave partial gradient / count sums in the
    ``[g || count]`` bucket: it is cleared here, and the next gradient launch is told
    the bucket is NOT known to be zero (it clears it itself), so no stale partial sum
    reaches an update or the sample count."""
    from dalgo.parallel import comm, xgmi
    if rt.is_main:
        print(f"[bench] device-side wait failed during {why}: falling back to per-step "
              f"launches over {rt.backend}", file=sys.stderr, flush=True)
    rt.synchronize()
    xgmi.disable()
    if hasattr(model, "bucket"):
        model.bucket.xg = None
        model.bucket.buffer.zero_()
    model._g_zero = False
    model._ok1, model._okp = False, False
    model.graph, model._okg = False, None
    model._graphs.clear()
    comm.reset_device_errors()
    rt.synchronize()
    rt.barrier()


def self_launch(a, argv) -> int | None:
    """``--gpus N`` without a launcher: N ranks as a torchrun child (dalgo.parallel.launch)."""
    from dalgo.parallel.launch import self_launch as _sl
    return _sl(a.gpus, __file__, argv, device=a.device, backend=a.backend, tag="bench")


def allreduce_probe(model, rt, iters: int = 100) -> float | None:
    """Per-step all-reduce cost in isolation (us, max over ranks): the SSGD/GD
    ``[g || count]`` bucket through whatever path the run uses (K11 or the process
    group). The bucket is all zeros between steps, so the probe leaves it unchanged."""
    from dalgo.parallel import comm
    if rt.world_size <= 1 or not hasattr(model, "bucket"):
        return None
    for _ in range(10):
        model.bucket.all_reduce()
    rt.synchronize()
    rt.barrier()
    t0 = time.perf_counter()
    for _ in range(iters):
        model.bucket.all_reduce()
    rt.synchronize()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=rt.device)
    comm.all_reduce_max(el)
    return float(el.item()) / iters * 1e6


def dump_outputs(path: str, model, rt, samples: float) -> None:
    """What a caller of the timed steps receives, as ``path/<name>.npy`` (rank 0 writes):
    the model after the last timed step (f32, replicated on every rank), the exact count
    of rows the timed steps sampled (f64) and, for MA / BMUF / EASGD, rank 0's local
    models. A few KB at the benchmark's sizes."""
    import numpy as np
    arrays = {"w": model.weights(),   # (completes a deferred EASGD centre update: every rank)
              "samples_counted": torch.tensor([samples], dtype=torch.float64)}
    if hasattr(model, "W"):
        arrays["locals_rank0"] = model.W
    rt.synchronize()
    if not rt.is_main:
        return
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach().cpu()
        t = t if t.dtype == torch.float64 else t.float()
        np.save(os.path.join(path, name + ".npy"), t.numpy())


def run_lr(a, rt, data, layout, algo: str, steps: int, warmup: int, witness_steps: int,
           calibrate: bool, dump_dir: str | None = None) -> dict:
    """One LR-family configuration on the shared data: warmup, optional launch-form
    calibration, EXACTLY ``steps`` timed training steps (barrier + synchronize on both
    sides, MAX over ranks; sampled rows counted on the device), the outputs of those steps
    to ``dump_dir`` if given, then (``--full``) the held-out witness (untimed: training
    continues to ``witness_steps`` total steps)."""
    from dalgo.models.localsgd import ParallelSGD, SGDConfig
    from dalgo.parallel import comm
    W = rt.world_size
    cfg = SGDConfig(algo=algo, n_workers=W, frac=a.frac, eval_every=0, n_iterations=steps)
    model = ParallelSGD(cfg, data, layout, rt)
    count = torch.zeros(1, dtype=torch.float64, device=rt.device)
    # model.run_steps(k): k full training steps, either k step() calls or (SSGD / GD with
    # DALGO_PERSISTENT=1) one persistent K1 launch running all k steps
    snap = model.state_dict()        # the untrained model: a fallback re-measures from here
    model.run_steps(warmup)
    rt.synchronize()
    cal = calibrate_launch(model, rt, a) if calibrate else {}

    def timed():
        rt.barrier()
        rt.synchronize()
        count.zero_()
        model.count_acc = count
        t_start = time.perf_counter()
        model.run_steps(steps)
        rt.synchronize()
        rt.barrier()
        rt.synchronize()
        el_ = time.perf_counter() - t_start
        n_ = model.global_sample_count()
        model.count_acc = None
        return el_, n_

    elapsed, samples = timed()
    if os.environ.get("DALGO_TEST_FORCE_DEVICE_ERROR") == str(rt.rank) and calibrate:
        # test hook: as if a wait of the timed region timed out, and as a launch that
        # stopped early would, leave partial sums in the gradient bucket
        comm._forced_error = 1
        if hasattr(model, "bucket"):
            model.bucket.buffer.fill_(1e3)
    fell_back = False
    # collective: MAX of every rank's device error words (K11 peer waits, persistent
    # step releases); if any wait timed out the timed steps are invalid: every rank
    # falls back to the plain per-step form and the warmup + timed region run again
    try:
        comm.check_device_errors("bench")
    except comm.DeviceCollectiveError:
        fallback_plain(model, rt, "the timed region")
        model.load_state_dict(snap)
        model.run_steps(warmup)
        elapsed, samples = timed()
        comm.check_device_errors("bench (fallback)")
        fell_back = True
    xg = getattr(getattr(model, "bucket", None), "xg", None)
    launch = "persistent" if model._persistent() else (
        "graph" if model._graph_ok() else (   # (the calibration's names: hipGraph replay = "graph")
            "one-kernel" if model._one_kernel() else "per-step"))
    allreduce = "xgmi-oneshot (K11)" if xg is not None else (
        f"{rt.backend}" if W > 1 else "none (1 rank)")
    el = torch.tensor([elapsed], dtype=torch.float64, device=rt.device)
    comm.all_reduce_max(el)
    elapsed = float(el.item())
    out = {"value": samples / elapsed, "ms_per_step": elapsed / steps * 1e3, "steps": steps,
           "warmup": warmup, "samples_counted": int(round(samples)),
           "global_batch": int(round(samples / steps)), "launch": launch, "allreduce": allreduce,
           "device_wait_fallback": fell_back}
    if cal:
        out["launch_calibration_ms_per_step"] = cal
    if dump_dir is not None:
        dump_outputs(dump_dir, model, rt, samples)
    out["allreduce_us_per_step"] = (allreduce_probe(model, rt)
                                    if a.full and algo in ("ssgd", "gd") else None)
    if a.eval:
        # correctness witness (untimed): train on to witness_steps and score the held-out
        # split against the planted model, whose own accuracy / log-loss on that split are
        # the Bayes ceiling / floor (WITNESS_TOL: how close each algorithm must come)
        done = warmup + steps
        extra = max(0, witness_steps - done)
        model.run_steps(extra)
        rt.synchronize()
        comm.check_device_errors("witness training")
        acc, loss = model.evaluate()
        from dalgo.data.datasets import planted_model
        ws = torch.from_numpy(planted_model(a.dim, 1234)).to(rt.device)
        d = model.data
        zs = d.X_test.float() @ ws[:a.dim] + ws[a.dim]
        bayes = float(((zs > 0).float() == d.y_test).float().mean().item())
        bayes_ll = float(torch.nn.functional.binary_cross_entropy_with_logits(zs, d.y_test.float()).item())
        tol_acc, tol_ll, why = WITNESS_TOL[algo]
        if tol_acc is None:   # MA / BMUF: half the way from chance to the ceiling
            tol_acc, why = 0.5 * (bayes - 0.5), "half the way from chance (0.5) to the planted accuracy"
        thr = bayes - tol_acc
        thr_ll = bayes_ll + tol_ll if tol_ll is not None else None
        out["correctness_witness"] = {
            "heldout_accuracy": acc, "heldout_logloss": loss, "n_test": a.n_test,
            "trained_steps": done + extra, "planted_model_accuracy": bayes,
            "planted_model_logloss": bayes_ll, "threshold": thr, "logloss_threshold": thr_ll,
            "tolerance": why,
            "passed": bool(acc >= thr and (thr_ll is None or loss <= thr_ll))}
    del model
    return out


# what the witnesses train to: the reference's iteration counts (ssgd.py:18, easgd.py:20),
# except MA / BMUF at 1500 rounds instead of 300 (ma.py:20, bmuf.py:20): BMUF's random
# initial block-momentum buffer (bmuf.py:95) adds sum_t 0.9^t Delta_0 = 10 Delta_0,
# Delta_0 ~ U[-1, 1), to every weight; at D = 1024 that takes more than 300 rounds to
# train away (held-out 0.56 at 300 rounds, 0.79 at 1500 on one MI355X). EASGD: 3000 rounds,
# its centre moves by beta = P alpha per round (easgd.py:24-25: 0.01 at P = 1)
REF_ITERS = {"ssgd": 1500, "gd": 1500, "ma": 1500, "bmuf": 1500, "easgd": 3000}

# (accuracy below the planted model's, log-loss above the planted model's, why): SSGD / GD /
# EASGD converge to the planted model at these step counts, so a gradient or update kernel
# that biases the model by more than ~2 points fails them. MA / BMUF carry the reference's
# random initial states (ma.py:86, bmuf.py:95) and start their rounds from them: their
# bound is half the way from chance to the ceiling, log-loss unchecked (BMUF's momentum
# keeps it above 2 at 1500 rounds)
WITNESS_TOL = {
    "ssgd": (0.02, 0.05, "within 0.02 of the planted accuracy, log-loss within 0.05 of it"),
    "gd": (0.02, 0.05, "within 0.02 of the planted accuracy, log-loss within 0.05 of it"),
    "easgd": (0.02, 0.08, "within 0.02 of the planted accuracy, log-loss within 0.08 of it"),
    "ma": (None, None, ""),
    "bmuf": (None, None, ""),
}


def run_secondary(a, rt, data, layout) -> dict:
    """BASELINE configs #3-#5 after the headline, inside a wall-clock budget: BMUF and
    EASGD on the headline's data (exact sampled-row counts, held-out witness at the
    reference's iteration counts), then -- with the LR data freed -- the k-means job
    (100M x 128, k = 1024; also on overlapping clusters) and the PageRank job (R-MAT scale
    26). A config whose start would come after the budget is recorded as skipped; a
    config that raises is recorded with its error (and fails the run)."""
    from dalgo.apps import jobs
    t0 = time.perf_counter()
    res = {}

    def budget_left():
        el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=rt.device)
        from dalgo.parallel import comm
        comm.all_reduce_max(el)
        return a.secondary_budget_s - float(el.item())

    def attempt(name, fn):
        if budget_left() <= 0:
            res[name] = {"skipped": f"secondary budget {a.secondary_budget_s:.0f} s spent"}
            return
        ts = time.perf_counter()
        try:
            r = fn()
        except Exception as e:   # noqa: BLE001 -- recorded; the run then exits non-zero
            import traceback
            traceback.print_exc()
            r = {"error": repr(e)}
        r["wall_s"] = time.perf_counter() - ts
        res[name] = r

    for algo in ("bmuf", "easgd"):
        attempt(algo, lambda algo=algo: dict(
            run_lr(a, rt, data, layout, algo, a.secondary_steps, a.secondary_warmup,
                   REF_ITERS[algo], calibrate=False),
            metric=f"samples/sec (whole node) {algo.upper()} logistic regression",
            unit="samples/s", config={"model": f"{algo.upper()} logistic regression",
                                      "rows": a.rows, "features": a.dim,
                                      "minibatch_fraction": a.frac,
                                      "parallelism": f"dp{rt.world_size}"}))
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    # ranks sharing one GPU (the one-GPU rehearsals) split its memory pool
    share = max(1, rt.world_size) if rt.shared_device else 1
    attempt("kmeans", lambda: jobs.kmeans_job(rt, a.km_rows, 128, 1024, 5, dtype=dt,
                                              pool_gb=a.km_pool_gb / share))
    attempt("kmeans_overlapping", lambda: jobs.kmeans_job(rt, a.km_rows, 128, 1024, 5, dtype=dt,
                                                          noise=a.km_hard_noise, warm=False,
                                                          pool_gb=a.km_pool_gb / share))
    attempt("pagerank", lambda: jobs.pagerank_job(rt, a.pr_scale, 16, 10, pool_gb=a.pr_pool_gb / share))
    return res


def secondary_failed(sec: dict) -> list:
    bad = []
    for k, v in sec.items():
        if "error" in v:
            bad.append(f"{k}: {v['error']}")
        w = v.get("correctness_witness")
        if w is not None and not w.get("passed", False):
            bad.append(f"{k}: witness failed")
    return bad


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    a = parse(argv)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    rc = self_launch(a, argv)
    if rc is not None:
        sys.exit(rc)
    from dalgo.data.datasets import synthetic_logistic
    from dalgo.parallel import runtime
    from dalgo.parallel.sharding import make_layout

    runtime.arm_watchdog(a.deadline_s, tag="bench")
    rt = runtime.init(backend=a.backend, device=a.device, app_name="bench-ssgd",
                      timeout_s=a.pg_timeout_s)
    W = rt.world_size
    from dalgo.parallel.launch import check_world
    check_world(a.gpus, W, "bench")
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    layout = make_layout(a.rows, W, W, rt.rank, spark_compatible=False)
    t0 = time.time()
    data = synthetic_logistic(a.rows, a.dim, row_range=(layout.row_lo, layout.row_hi),
                              n_test=a.n_test if a.eval else 0, device=rt.device, dtype=dtype)
    rt.synchronize()
    gen_s = time.time() - t0
    head = run_lr(a, rt, data, layout, a.algo, a.steps, a.warmup, a.witness_steps,
                  calibrate=a.launch == "auto",
                  dump_dir=os.path.abspath(a.dump_outputs) if a.dump_outputs else None)
    sec_on = a.secondary == "on" or (a.secondary == "auto" and rt.device.type == "cuda")
    sec = run_secondary(a, rt, data, layout) if sec_on else None
    value = head["value"]
    witness = head.get("correctness_witness")
    if rt.is_main:
        out = {
            "metric": BASELINE_METRIC,
            "value": value,
            "unit": "samples/s",
            "n_gpus": W,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": head["ms_per_step"],
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": (value / BASELINE_VALUE) if BASELINE_VALUE else None,
            "dtype": a.dtype,
            "data": f"synthetic (on-device Philox planted logistic model, {a.rows}x{a.dim}, random-init w)",
            "config": {"model": f"{a.algo.upper()} logistic regression", "global_batch": head["global_batch"],
                       "seq_len": None, "features": a.dim, "rows": a.rows,
                       "minibatch_fraction": a.frac, "parallelism": f"dp{W}",
                       "allreduce": head["allreduce"], "launch": head["launch"]},
            "samples_counted": head["samples_counted"],
            "per_gpu_samples_per_s": value / W,
            "effective_hbm_GBps_per_gpu": value / W * a.dim * (2 if dtype == torch.bfloat16 else 4) / 1e9,
            "datagen_s": gen_s,
            "full": a.full,
        }
        if "launch_calibration_ms_per_step" in head:
            out["launch_calibration_ms_per_step"] = head["launch_calibration_ms_per_step"]
        from dalgo.parallel import xgmi
        out["world_size"] = W
        out["device_ids"] = list(rt.device_ids)
        out["distinct_devices"] = len(set(rt.device_ids))
        out["shared_device"] = rt.shared_device
        out["backend"] = rt.backend
        if rt.device.type == "cuda":
            try:
                out["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                out["rccl_version"] = None
        out["small_allreduce_race"] = xgmi.last_race
        out["device_wait_fallback"] = head["device_wait_fallback"]
        out["allreduce_us_per_step"] = head["allreduce_us_per_step"]
        if witness is not None:
            out["heldout_accuracy"] = witness["heldout_accuracy"]
            out["correctness_witness"] = witness
        if sec is not None:
            out["secondary"] = sec
        print(json.dumps(out), flush=True)
    runtime.shutdown()
    runtime.arm_watchdog(0)
    if witness is not None and not witness["passed"]:
        raise SystemExit(f"[bench] correctness witness failed: held-out accuracy "
                         f"{witness['heldout_accuracy']:.4f} < {witness['threshold']:.4f}")
    bad = secondary_failed(sec or {})
    if bad:
        raise SystemExit("[bench] secondary config failed: " + "; ".join(bad))


if __name__ == "__main__":
    main()
