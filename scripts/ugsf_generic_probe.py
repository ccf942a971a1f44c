"""Ad-hoc: throughput of the run-time-dimension unscented Gaussian-sum filter (csrc/ugsf_generic.hip) on Lorenz-96 with the
even-state emission, K = 4, no output streams and all five, next to the extended filter (gaussian_sum_filter: matrix-core or
run-time-dimension kernels, O(n^3) per step without an eigen-decomposition) at the same shape and batch.  The ratio is context,
not a target.  B fills the device (one workgroup per trajectory); T is scaled from a short calibration run to a few hundred
milliseconds.  Observations come from the model itself (device generator), and the share of finite final means is printed:
a filter that has gone NaN leaves the Jacobi loop at once and would look fast.

  python scripts/ugsf_generic_probe.py            # all shapes
  python scripts/ugsf_generic_probe.py 16 8       # one shape, one timed call per filter (for a kernel trace)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bayesianfiltering_amd as bfa
from oracle import threefry as otf

F32 = np.float32
K = 4
nl = bfa.nonlinearities
shapes = ((12, 6, 8192), (16, 8, 8192), (24, 12, 4096), (40, 20, 1024))
one = len(sys.argv) == 3
if one:
    shapes = tuple(s for s in shapes if s[:2] == (int(sys.argv[1]), int(sys.argv[2])))


def timed(fn):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


for n, m, B in shapes:
    p = bfa.ParamsNLSSM(8 * np.ones(n, F32), np.eye(n, dtype=F32), nl.lorenz96(n), np.zeros(n, F32), 1e-2 * np.eye(n, dtype=F32),
                        nl.pick_even(n), np.zeros(m, F32), 1e-1 * np.eye(m, dtype=F32))
    up = bfa.ParamsUKF(1, 0, 0)
    init = torch.as_tensor((8 + np.random.default_rng(n).normal(size=(B, K, n))).astype(F32), device="cuda")
    keys = otf.split(otf.PRNGKey(n), B)
    cal = 4
    ycal = bfa.NonlinearSSM(n, n, m, m).sample(p, keys, cal)[1]
    bfa.unscented_gaussian_sum_filter(p, up, ycal, K, 1, initial_means=init, fields=())      # first call: module load, constants
    ms, _ = timed(lambda: bfa.unscented_gaussian_sum_filter(p, up, ycal, K, 1, initial_means=init, fields=(), return_carry=True))
    cap = int(4e9 / (B * K * 2 * n * n * 4))                                                   # FULL5 streams stay under 4 GB
    T = max(8, min(int(300.0 / (ms / cal)), cap, 400))
    y = bfa.NonlinearSSM(n, n, m, m).sample(p, keys, T)[1]
    for fields, name in (((), "none"), (bfa.FULL5, "FULL5")):
        for filt, run in (("unscented", lambda f, o: bfa.unscented_gaussian_sum_filter(p, up, y, K, 1, initial_means=init, fields=f, out=o, return_carry=True)),
                          ("extended ", lambda f, o: bfa.gaussian_sum_filter(p, y, K, 1, initial_means=init, fields=f, out=o, return_carry=True))):
            post, carry = run(fields, None)                                                    # warm-up, allocates the streams
            ms, (post, carry) = timed(lambda: run(fields, post))
            fin = float(torch.isfinite(carry[1]).all(dim=2).float().mean())
            print(f"{filt} n={n:3d} m={m:3d} K={K} B={B} T={T} {name:5s}: {ms:9.2f} ms  {B * K * T / ms / 1e3:9.3f} M component-steps/s"
                  f"  finite {fin:.3f}", flush=True)
            if one:
                break
        if one:
            break
