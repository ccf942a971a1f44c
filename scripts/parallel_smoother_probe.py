"""Ad-hoc: parallel_rts_smoother against rts_smoother (the yardstick) on the same filter streams.  Model n = 4, m = 2 (the
stable random model "4x2" of tests/parallel_kalman_cases.py), both routes -- the predictions given, and recomputed from the filtered streams --, smoothed means and
covariances, contiguous reference layout, output buffers and workspace allocated once (out= / workspace=).  B = 1 / T = 10^6 with
the block length swept over 16 ... 1024, then B = 64 / T = 10^5, B = 1 024 / T = 10^4 and B = 65 536 / T = 10^3 at a few block
lengths and the default.  Per case: 2 warm-up and 7 timed runs with device events in one process (the serial smoother on 10^6
steps: 1 and 3); the table shows the median and the spread (min ... max) in ms, trajectory-steps/s from the median, the bytes
the call stores per second, and the ratio of the serial smoother's median to the parallel one's; the last column is rel_err of
the smoothed means of trajectory 0 over its last 3000 steps against the float64 recursion on the same fp32 streams
(tests/test_smoother_cpu.py: rts_f64; the smoother of a suffix reads nothing before it).

  python scripts/parallel_smoother_probe.py [--out FILE]        # the table (default profiles/parallel_smoother_probe.txt)
  python scripts/parallel_smoother_probe.py --one B T L [given]  # the parallel smoother alone, a few runs (for a kernel trace)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bayesianfiltering_amd as bfa
from tests import common as cm
from tests import parallel_smoother_cases as psc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "parallel_smoother_probe.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return float(np.median(ms)), min(ms), max(ms)


a = psc.model("4x2")   # stable: on the constant-velocity model the fp32 filter's covariances drift over 10^6 steps until the
                        # float64 yardstick's Cholesky refuses a predicted covariance
params = cm.product_params(a)
n = 4
BYTES_STORED = 4 * (n + n * n)   # smoothed mean and covariance per trajectory-step
CHECK = 3000


def filtered(B, T):
    """the FULL5 streams of kalman_filter on the model's own data for a short stretch, tiled in time"""
    base = cm.simulate_batch(a, min(B, 64), min(T, 4096), seed=9)
    y = torch.as_tensor(base, device="cuda")
    y = y.repeat((B + y.shape[0] - 1) // y.shape[0], (T + y.shape[1] - 1) // y.shape[1], 1)[:B, :T].contiguous()
    return bfa.kalman_filter(params, y)


def case(B, T, blocks):
    full = filtered(B, T)
    C_ = min(T, CHECK)
    tail = [getattr(full, k)[0, 0, T - C_:].cpu().numpy() for k in ("means", "covariances", "predicted_means", "predicted_covariances")]
    f64 = psc.rts_f64(*tail, a["A"])[0]
    for route, post in (("given", full), ("recomputed", full._replace(predicted_means=None, predicted_covariances=None))):
        sm = bfa.rts_smoother(params, post)
        seq = lambda: bfa.rts_smoother(params, post, out=sm)
        long_run = T >= 500_000
        s_med, s_min, s_max = timed(seq, 1 if long_run else 2, 3 if long_run else 7)
        s_err = cm.rel_err(sm.smoothed_means[0, 0, T - C_:].cpu().numpy(), f64)
        say(f"B={B:6d} T={T:8d} {route:10s} rts_smoother             {s_med:10.3f} ms ({s_min:.3f} ... {s_max:.3f})  {B * T / s_med * 1e3:9.3e} steps/s"
            f"  {B * T * BYTES_STORED / s_med / 1e9:6.3f} TB/s stored             means vs float64 {s_err:.1e}")
        for L in blocks:
            ws = torch.empty(bfa.parallel_rts_workspace_bytes(n, B, T, L), dtype=torch.uint8, device="cuda")
            par = lambda: bfa.parallel_rts_smoother(params, post, out=sm, block=L, workspace=ws)
            p_med, p_min, p_max = timed(par, 2, 7)
            err = cm.rel_err(sm.smoothed_means[0, 0, T - C_:].cpu().numpy(), f64)
            name = "default" if L is None else f"{L:7d}"
            say(f"B={B:6d} T={T:8d} {route:10s} parallel block={name}    {p_med:10.3f} ms ({p_min:.3f} ... {p_max:.3f})  {B * T / p_med * 1e3:9.3e} steps/s"
                f"  {B * T * BYTES_STORED / p_med / 1e9:6.3f} TB/s stored  x{s_med / p_med:8.2f}  means vs float64 {err:.1e}")
            del ws
        del sm
    del full
    torch.cuda.empty_cache()


if args[:1] == ["--one"]:
    B, T, L = int(args[1]), int(args[2]), int(args[3])
    post = filtered(B, T)
    if args[4:5] != ["given"]:
        post = post._replace(predicted_means=None, predicted_covariances=None)
    sm = bfa.parallel_rts_smoother(params, post, block=L)
    ws = torch.empty(bfa.parallel_rts_workspace_bytes(n, B, T, L), dtype=torch.uint8, device="cuda")
    for _ in range(4):
        bfa.parallel_rts_smoother(params, post, out=sm, block=L, workspace=ws)
    torch.cuda.synchronize()
    sys.exit(0)

say(f"device: {torch.cuda.get_device_name(0)}; n={n}; {BYTES_STORED} bytes stored per trajectory-step (smoothed mean and covariance); "
    "times are medians (min ... max)")
case(1, 1_000_000, (16, 32, 64, 128, 256, 512, 1024, None))
for B, T in ((64, 100_000), (1024, 10_000), (65536, 1_000)):
    case(B, T, (16, 64, 256, None))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
