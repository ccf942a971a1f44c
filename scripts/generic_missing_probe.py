"""Ad-hoc: what missing observations cost on the run-time-dimension kernel (csrc/generic_device.hpp, MISSING = true;
DESIGN.md 4a'').  Two shapes -- a linear model (n = 12, m = 4, K = 1) and Lorenz-96 with the even-state emission (n = 12, m = 6,
K = 4) -- at B = 16 384 trajectories, T = 1 000 steps, all five streams plus nothing else.  Three variants alternate over the
rounds, each one timed call on the same buffers:

  plain      the plain kernel on complete data             (options={"force_generic": 1})
  complete   the new route, nothing missing                (missing="nan" on the same data)
  gaps       the new route, 30 % of the entries missing    (independently per entry)

Reported per shape: the median time of each variant, the plain kernel's own round-to-round spread ((max - min) / median), and the
two ratios complete / plain and gaps / complete.  One more line: a linear (32, 16) model with 30 % gaps on the new route against
the plain call (matrix-core kernel) on the complete data -- the factor a gapped model pays for leaving that route.

  python scripts/generic_missing_probe.py [B] [T] [rounds]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bayesianfiltering_amd as bfa
from oracle import threefry as otf

F32 = np.float32
nl = bfa.nonlinearities
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
GENERIC = {"force_generic": 1}


def timed(fn):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def linear_model(n, m):
    """A stable banded A, the first m states observed through a banded H, well-conditioned Q, R, P0."""
    A = (0.9 * np.eye(n) + 0.05 * np.eye(n, k=1) - 0.04 * np.eye(n, k=-1)).astype(F32)
    H = (np.eye(m, n) + 0.1 * np.eye(m, n, k=1)).astype(F32)
    return bfa.ParamsNLSSM(np.zeros(n, F32), np.eye(n, dtype=F32), nl.linear_dynamics(A), np.zeros(n, F32), 0.1 * np.eye(n, dtype=F32),
                           nl.linear_emission(H), np.zeros(m, F32), 0.2 * np.eye(m, dtype=F32))


def lorenz96_model(n):
    m = n // 2
    return bfa.ParamsNLSSM(8 * np.ones(n, F32), np.eye(n, dtype=F32), nl.lorenz96(n), np.zeros(n, F32), 1e-2 * np.eye(n, dtype=F32),
                           nl.pick_even(n), np.zeros(m, F32), 1e-1 * np.eye(m, dtype=F32))


def gapped(y, share, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.where(torch.rand(y.shape, device="cuda", generator=g) < share, torch.full((), float("nan"), device="cuda"), y)


def observations(p, n, m, Bn, Tn):
    return bfa.NonlinearSSM(n, n, m, m).sample(p, otf.split(otf.PRNGKey(n + m), Bn), Tn)[1]


def run(p, y, K, init, kalman, out, **kw):
    if kalman:
        return bfa.kalman_filter(p, y, initial_means=init, out=out, return_carry=True, **kw)
    return bfa.gaussian_sum_filter(p, y, K, 1, initial_means=init, out=out, return_carry=True, **kw)


def shape_report(label, p, n, m, K, kalman):
    y = observations(p, n, m, B, T)
    yg = gapped(y, 0.3, 1)
    m0 = np.asarray(p.initial_mean, F32)
    init = torch.as_tensor((m0 + np.random.default_rng(n).normal(size=(B, K, n))).astype(F32), device="cuda")
    if kalman:
        init = init[:, 0]
    variants = (("plain", y, dict(options=GENERIC)), ("complete", y, dict(missing="nan", options=GENERIC)),
                ("gaps", yg, dict(missing="nan", options=GENERIC)))
    post = None
    for _, ys, kw in variants:                                   # warm-up: code objects, constants, the streams
        post, _ = run(p, ys[:, :8], K, init, kalman, None, **kw)
    post, _ = run(p, y, K, init, kalman, None, options=GENERIC)
    ms = {name: [] for name, _, _ in variants}
    fin = {}
    for _ in range(ROUNDS):
        for name, ys, kw in variants:
            t, (post, carry) = timed(lambda: run(p, ys, K, init, kalman, post, **kw))
            ms[name].append(t)
            fin[name] = float(torch.isfinite(carry[1]).all(dim=2).float().mean())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = (max(ms["plain"]) - min(ms["plain"])) / med["plain"]
    print(f"{label}: B={B} T={T} K={K}, five streams, {ROUNDS} rounds")
    for name in ms:
        print(f"  {name:9s} median {med[name]:9.2f} ms  ({B * K * T / med[name] / 1e3:8.2f} M component-steps/s)  rounds "
              + " ".join(f"{v:.2f}" for v in ms[name]) + f"  finite {fin[name]:.3f}")
    print(f"  plain kernel's round-to-round spread {100 * spread:.2f} %;  complete / plain = {med['complete'] / med['plain']:.4f};  "
          f"gaps / complete = {med['gaps'] / med['complete']:.4f}", flush=True)
    del post, y, yg
    torch.cuda.empty_cache()


shape_report("linear (12, 4)", linear_model(12, 4), 12, 4, 1, True)
shape_report("lorenz96 (12, 6)", lorenz96_model(12), 12, 6, 4, False)

# the factor for leaving the matrix-core route: (32, 16), a quarter of the horizon (2 113 floats per step and trajectory)
n, m, Tq = 32, 16, max(8, T // 4)
p = linear_model(n, m)
y = observations(p, n, m, B, Tq)
yg = gapped(y, 0.3, 2)
init = torch.as_tensor(np.random.default_rng(n).normal(size=(B, n)).astype(F32), device="cuda")
calls = (("plain call, complete data (matrix cores)", lambda o: bfa.kalman_filter(p, y, initial_means=init, out=o)),
         ("plain run-time-dimension kernel, complete", lambda o: bfa.kalman_filter(p, y, initial_means=init, out=o, options=GENERIC)),
         ("new route, 30 % missing", lambda o: bfa.kalman_filter(p, yg, initial_means=init, out=o, missing="nan")))
post = calls[0][1](None)
for _, call in calls:
    call(post)
ms = {name: [] for name, _ in calls}
for _ in range(ROUNDS):
    for name, call in calls:
        ms[name].append(timed(lambda: call(post))[0])
med = {k: float(np.median(v)) for k, v in ms.items()}
print(f"linear (32, 16): B={B} T={Tq} K=1, five streams, {ROUNDS} rounds")
for name in ms:
    print(f"  {name:42s} median {med[name]:9.2f} ms  ({B * Tq / med[name] / 1e3:8.2f} M steps/s)")
names = [name for name, _ in calls]
print(f"  gapped on the new route / plain call on the matrix cores = {med[names[2]] / med[names[0]]:.2f};  "
      f"gapped / plain run-time-dimension kernel = {med[names[2]] / med[names[1]]:.4f}")
