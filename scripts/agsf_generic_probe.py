"""Ad-hoc: throughput of the run-time-dimension augmented Gaussian-sum filters (csrc/agsf_generic.hip) on Lorenz-96 with the
even-state emission, trees (3, 2, 2) and (4, 4, 4), extended and unscented nodes, in leaf-steps/s (B x N0 N1 N2 x T / time).
Beside it, as context and not as a target: gaussian_sum_filter on its run-time-dimension kernel (options={"force_generic": 1})
with K = N0 N1 N2 components at the same shape, batch and length -- the same number of node updates, no tree -- and, at
(n, m) = (8, 4), the register kernel (a leaf per lane) against options={"agsf_force_generic": 1}.  Observations come from the
model itself (device generator); the share of trajectories whose final carried means are finite is printed with every figure: a
filter that has gone NaN would look fast.  T is scaled from a two-step calibration run to about 150 ms, 40 steps at the most.

  python scripts/agsf_generic_probe.py [--out FILE]          # all shapes; the table goes to FILE (default profiles/agsf_generic_probe.txt)
  python scripts/agsf_generic_probe.py 16 8                  # one shape, one tree, the two node kinds only (for a kernel trace, or with
                                                             # BAYESFILT_AGSF_NT64_MAX set, for the workgroup-size threshold)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bayesianfiltering_amd as bfa
from oracle import threefry as otf

F32 = np.float32
nl = bfa.nonlinearities
args = sys.argv[1:]
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "agsf_generic_probe.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i:i + 2]
shapes = ((12, 6, 8192), (16, 8, 8192), (24, 12, 2048), (40, 20, 512))
trees = ((3, 2, 2), (4, 4, 4))
one = len(args) == 2
if one:
    shapes = tuple(s for s in shapes if s[:2] == (int(args[0]), int(args[1]))) or ((int(args[0]), int(args[1]), 1024),)
    trees = trees[:1]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def model(n, m):
    return bfa.ParamsNLSSM(8 * np.ones(n, F32), np.eye(n, dtype=F32), nl.lorenz96(n), np.zeros(n, F32), 1e-2 * np.eye(n, dtype=F32),
                           nl.pick_even(n), np.zeros(m, F32), 1e-1 * np.eye(m, dtype=F32))


def finite_share(carry):
    return float(torch.isfinite(carry[1]).all(dim=2).all(dim=1).float().mean())


def agsf(p, up, y, nc, init, options=None):
    if up is None:
        return bfa.speedy_augmented_gaussian_sum_filter(p, y, nc, initial_means=init, return_carry=True, options=options)[1]["carry"]
    return bfa.speedy_unscented_agsf(p, up, y, nc, initial_means=init, return_carry=True, options=options)[1]["carry"]


def length(run, sample, B):
    cal = 2
    ycal = sample(cal)
    run(ycal)                                                 # first call: module load, constants
    ms, _ = timed(lambda: run(ycal))
    return max(4, min(int(150.0 / (ms / cal)), 40))     # (long Lorenz-96 runs lose a trajectory in a hundred to divergence, in every kernel)


up = bfa.ParamsUKF(1, 0, 0)
for n, m, B in shapes:
    p = model(n, m)
    keys = otf.split(otf.PRNGKey(n), B)
    sample = lambda T: bfa.NonlinearSSM(n, n, m, m).sample(p, keys, T)[1]
    for nc in trees:
        M = int(np.prod(nc))
        init = torch.as_tensor((8 + np.random.default_rng(n).normal(size=(B, nc[0], n))).astype(F32), device="cuda")
        for nodes, u in (("extended ", None), ("unscented", up)):
            T = length(lambda yy: agsf(p, u, yy, nc, init), sample, B)
            y = sample(T)
            ms, carry = timed(lambda: agsf(p, u, y, nc, init))
            say(f"agsf {nodes} n={n:3d} m={m:3d} tree={nc} B={B} T={T:3d}: {ms:9.2f} ms  {B * M * T / ms / 1e3:9.3f} M leaf-steps/s"
                f"  finite {finite_share(carry):.3f}")
            if u is None and not one:     # context: the Gaussian-sum filter's run-time-dimension kernel doing K = M node updates per step
                initK = torch.as_tensor((8 + np.random.default_rng(n).normal(size=(B, M, n))).astype(F32), device="cuda")
                gsf = lambda yy: bfa.gaussian_sum_filter(p, yy, M, 1, initial_means=initK, fields=(), return_carry=True,
                                                         options={"force_generic": 1})[1]
                gsf(y[:, :2])
                ms, carry = timed(lambda: gsf(y))
                say(f"gsf  generic   n={n:3d} m={m:3d} K={M:9d} B={B} T={T:3d}: {ms:9.2f} ms  {B * M * T / ms / 1e3:9.3f} M component-steps/s"
                    f"  finite {finite_share(carry):.3f}")

if not one:   # the two kernels on the register kernel's ground
    n, m, B = 8, 4, 8192
    p = model(n, m)
    keys = otf.split(otf.PRNGKey(n), B)
    sample = lambda T: bfa.NonlinearSSM(n, n, m, m).sample(p, keys, T)[1]
    for nc in trees:
        M = int(np.prod(nc))
        init = torch.as_tensor((8 + np.random.default_rng(n).normal(size=(B, nc[0], n))).astype(F32), device="cuda")
        T = length(lambda yy: agsf(p, None, yy, nc, init, {"agsf_force_generic": 1}), sample, B)
        y = sample(T)
        for name, opt in (("register kernel ", None), ("run-time-dim.   ", {"agsf_force_generic": 1})):
            agsf(p, None, y[:, :2], nc, init, opt)
            ms, carry = timed(lambda: agsf(p, None, y, nc, init, opt))
            say(f"agsf extended  n={n:3d} m={m:3d} tree={nc} B={B} T={T:3d} {name}: {ms:9.2f} ms  {B * M * T / ms / 1e3:9.3f} M leaf-steps/s"
                f"  finite {finite_share(carry):.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
