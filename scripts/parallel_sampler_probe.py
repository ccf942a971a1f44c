"""Ad-hoc: parallel_posterior_sample against posterior_sample (the yardstick) on the same filter streams and noise.  Model n = 4,
m = 2 (the stable random model "4x2" of tests/parallel_kalman_cases.py), both routes -- the predictions given, and recomputed
from the filtered streams --, noise given as a stream, contiguous reference layout, the sample buffer and workspace allocated once
(out= / workspace=).  (B, S, T) = (1, 1, 10^6) and (1, 16, 10^6) with the block length swept over 16 ... 1024, then (64, 4, 10^5),
(1024, 4, 10^4) and (65 536, 1, 256) at a few block lengths, each with the default and with the block length the parallel
filter's rule gives for (B S, T) (marked *: the default before this sweep); one key-mode row at (1, 1, 10^6).  Per case:
2 warm-up and 7 timed runs with device events in one process (the serial sampler on 10^6 steps: 1 and 3); the table shows the
median and the spread (min ... max) in ms, sample-steps/s from the median, the bytes the call stores per second, and the ratio of
the serial sampler's median to the parallel one's; the last column is the error (tests/test_sampler_gpu.py: _err) of the samples
of trajectory 0 over its last 3000 steps against the float64 recursion on the same fp32 streams and noise
(tests/test_sampler_cpu.py: ffbs_f64; the sampler of a suffix reads nothing before it).

  python scripts/parallel_sampler_probe.py [--out FILE]           # the table (default profiles/parallel_sampler_probe.txt)
  python scripts/parallel_sampler_probe.py --one B S T L [given]  # the parallel sampler alone, a few runs (for a kernel trace)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bayesianfiltering_amd as bfa
from tests import common as cm
from tests import parallel_sampler_cases as psc
from tests.test_sampler_gpu import _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "parallel_sampler_probe.txt")
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


a = psc.model("4x2")   # stable: on the constant-velocity model the fp32 filter's covariances drift over 10^6 steps
params = cm.product_params(a)
n = 4
BYTES_STORED = 4 * n   # one sample per (trajectory, sample, step)
CHECK = 3000
STREAMS = ("means", "covariances", "predicted_means", "predicted_covariances")


def filtered(B, T):
    """the FULL5 streams of kalman_filter on the model's own data for a short stretch, tiled in time"""
    base = cm.simulate_batch(a, min(B, 64), min(T, 4096), seed=9)
    y = torch.as_tensor(base, device="cuda")
    y = y.repeat((B + y.shape[0] - 1) // y.shape[0], (T + y.shape[1] - 1) // y.shape[1], 1)[:B, :T].contiguous()
    return bfa.kalman_filter(params, y)


def filter_rule(B, T):
    """the parallel filter's default block for (B, T): the largest of ceil(B T / 65 536), the smallest s with 50 s^2 >= T, and 16"""
    s = next(s for s in range(1, 4097) if 50 * s * s >= T or s == 4096)
    return min(max(-(-B * T // 65536), s, 16), 4096)


def row(B, S, T, route, what, med, lo, hi, ratio, err):
    steps = B * S * T
    say(f"B={B:6d} S={S:3d} T={T:8d} {route:10s} {what:26s} {med:10.3f} ms ({lo:.3f} ... {hi:.3f})  {steps / med * 1e3:9.3e} sample-steps/s"
        f"  {steps * BYTES_STORED / med / 1e9:6.3f} TB/s stored  {ratio:>9s}  samples vs float64 {err:.1e}")


def case(B, S, T, blocks, keyed_row=False):
    full = filtered(B, T)
    xi = torch.randn((B, S, T, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(17))
    C_ = min(T, CHECK)
    tail = full._replace(**{k: getattr(full, k)[:1, :, T - C_:] for k in ("weights",) + STREAMS})
    f64 = psc.ffbs_f64(*(getattr(tail, k)[0, 0].cpu().numpy() for k in STREAMS), a["A"], xi[0, :, T - C_:].cpu().numpy())
    err_of = lambda x: _err(x[0, :, T - C_:].cpu().numpy(), f64, tail)
    long_run = T >= 500_000
    for route, post in (("given", full), ("recomputed", full._replace(predicted_means=None, predicted_covariances=None))):
        x = bfa.posterior_sample(params, post, S, noise=xi)
        s_med, s_min, s_max = timed(lambda: bfa.posterior_sample(params, post, S, noise=xi, out=x), 1 if long_run else 2, 3 if long_run else 7)
        row(B, S, T, route, "posterior_sample", s_med, s_min, s_max, "", err_of(x))
        for L in tuple(blocks) + (-filter_rule(B * S, T),):
            name = "default" if L is None else f"{abs(L):7d}" if L > 0 else f"{abs(L):6d}*"
            L = None if L is None else abs(L)
            ws = torch.empty(bfa.parallel_ffbs_workspace_bytes(n, B, T, S, L), dtype=torch.uint8, device="cuda")
            par = lambda: bfa.parallel_posterior_sample(params, post, S, noise=xi, out=x, block=L, workspace=ws)
            p_med, p_min, p_max = timed(par, 2, 7)
            row(B, S, T, route, f"parallel block={name}", p_med, p_min, p_max, f"x{s_med / p_med:8.2f}", err_of(x))
            del ws
        if keyed_row and route == "recomputed":
            key = bfa.PRNGKey(3)
            k_med, k_min, k_max = timed(lambda: bfa.posterior_sample(params, post, S, key=key, out=x), 1, 3)
            say(f"B={B:6d} S={S:3d} T={T:8d} {route:10s} posterior_sample, key      {k_med:10.3f} ms ({k_min:.3f} ... {k_max:.3f})")
            p_med, p_min, p_max = timed(lambda: bfa.parallel_posterior_sample(params, post, S, key=key, out=x), 2, 7)
            say(f"B={B:6d} S={S:3d} T={T:8d} {route:10s} parallel default, key      {p_med:10.3f} ms ({p_min:.3f} ... {p_max:.3f})  x{k_med / p_med:8.2f}")
        del x
    del full, xi
    torch.cuda.empty_cache()


if args[:1] == ["--one"]:
    B, S, T, L = (int(v) for v in args[1:5])
    post = filtered(B, T)
    if args[5:6] != ["given"]:
        post = post._replace(predicted_means=None, predicted_covariances=None)
    xi = torch.randn((B, S, T, n), device="cuda")
    x = bfa.parallel_posterior_sample(params, post, S, noise=xi, block=L)
    ws = torch.empty(bfa.parallel_ffbs_workspace_bytes(n, B, T, S, L), dtype=torch.uint8, device="cuda")
    for _ in range(4):
        bfa.parallel_posterior_sample(params, post, S, noise=xi, out=x, block=L, workspace=ws)
    torch.cuda.synchronize()
    sys.exit(0)

say(f"device: {torch.cuda.get_device_name(0)}; n={n}; {BYTES_STORED} bytes stored per sample-step; times are medians (min ... max); "
    "block=L*: the parallel filter's rule on (B S, T)")
case(1, 1, 1_000_000, (16, 32, 64, 128, 256, 512, 1024, None), keyed_row=True)
case(1, 16, 1_000_000, (16, 32, 64, 128, 256, 512, 1024, None))
for B, S, T in ((64, 4, 100_000), (1024, 4, 10_000), (65536, 1, 256)):
    case(B, S, T, (16, 64, 256, None))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
