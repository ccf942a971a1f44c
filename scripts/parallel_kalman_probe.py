"""Ad-hoc: parallel_kalman_filter against kalman_filter on few long trajectories.  Model n = 4, m = 2 (the headline
constant-velocity model), all five streams plus the log-likelihood, contiguous reference layout, identical emissions, output
buffers and workspace allocated once (out= / workspace=).  B in {1, 8, 64, 1024, 65 536}; T = 10^6 reduced at large B so that
the streams fit; block lengths 16, 64, 256 and the default.  Per case: warm-up runs, then timed runs with device events in one
process; the table shows the median and the spread (min ... max) in ms, trajectory-steps/s from the median, and the ratio of the
sequential filter's median to the parallel one's; the last column is rel_err of the means of trajectory 0 over its first
3000 steps against the float64 recursion (tests/parallel_kalman_cases.py).

  python scripts/parallel_kalman_probe.py [--out FILE]     # the table (default profiles/parallel_kalman_probe.txt)
  python scripts/parallel_kalman_probe.py --one B T L      # the parallel filter alone, a few runs (for a kernel trace)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bayesianfiltering_amd as bfa
from tests import common as cm
from tests import parallel_kalman_cases as pk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "parallel_kalman_probe.txt")
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


a = cm.cv_model_arrays()
params = cm.product_params(a)
n, m = 4, 2
BYTES_PER_STEP = 4 * (1 + 2 * n + 2 * n * n + 1)   # what the enabled streams store per trajectory-step
CHECK = 3000


def emissions(B, T):
    """device observations: the model's own data for a short stretch, tiled in time (the filters' cost does not depend on the values)"""
    base = cm.simulate_batch(a, min(B, 64), min(T, 4096), seed=9)
    y = torch.as_tensor(base, device="cuda")
    y = y.repeat((B + y.shape[0] - 1) // y.shape[0], (T + y.shape[1] - 1) // y.shape[1], 1)[:B, :T].contiguous()
    return y


def case(B, T, blocks):
    y = emissions(B, T)
    post, ll = bfa.kalman_filter(params, y, return_loglik=True)
    seq = lambda: bfa.kalman_filter(params, y, out=post)
    long_run = T >= 500_000
    s_med, s_min, s_max = timed(seq, 1, 3 if long_run else 7)
    # both filters against the float64 recursion over the first CHECK steps of trajectory 0
    C_ = min(T, CHECK)
    f64 = pk.kalman_f64(a, y[:1, :C_].cpu().numpy(), a["m0"][None], a["P0"])["means"]
    s_err = cm.rel_err(post.means[:1, :, :C_].cpu().numpy(), f64)
    say(f"B={B:6d} T={T:8d}  kalman_filter            {s_med:10.3f} ms ({s_min:.3f} ... {s_max:.3f})  {B * T / s_med * 1e3:9.3e} steps/s"
        f"  means vs float64 {s_err:.1e}")
    for L in blocks:
        ws = torch.empty(bfa.parallel_kalman_workspace_bytes(n, m, B, T, L), dtype=torch.uint8, device="cuda")
        par = lambda: bfa.parallel_kalman_filter(params, y, out=post, block=L, workspace=ws)
        p_med, p_min, p_max = timed(par, 2, 7)
        err = cm.rel_err(post.means[:1, :, :C_].cpu().numpy(), f64)
        name = "default" if L is None else f"{L:7d}"
        say(f"B={B:6d} T={T:8d}  parallel block={name}   {p_med:10.3f} ms ({p_min:.3f} ... {p_max:.3f})  {B * T / p_med * 1e3:9.3e} steps/s"
            f"  {B * T * BYTES_PER_STEP / p_med / 1e9:6.3f} TB/s stored  x{s_med / p_med:8.2f}  means vs float64 {err:.1e}")
        del ws
    del post, ll, y
    torch.cuda.empty_cache()


if args[:1] == ["--one"]:
    B, T, L = int(args[1]), int(args[2]), int(args[3])
    y = emissions(B, T)
    post = bfa.parallel_kalman_filter(params, y, block=L)
    ws = torch.empty(bfa.parallel_kalman_workspace_bytes(n, m, B, T, L), dtype=torch.uint8, device="cuda")
    for _ in range(4):
        bfa.parallel_kalman_filter(params, y, out=post, block=L, workspace=ws)
    torch.cuda.synchronize()
    sys.exit(0)

say(f"device: {torch.cuda.get_device_name(0)}; n={n}, m={m}; {BYTES_PER_STEP} bytes stored per trajectory-step; times are medians (min ... max)")
for B, T in ((1, 1_000_000), (8, 1_000_000), (64, 100_000), (1024, 10_000), (65536, 256)):
    case(B, T, (16, 64, 256, None))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
