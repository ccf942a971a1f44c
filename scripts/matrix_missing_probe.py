"""Ad-hoc: what missing observations cost on the one-wave matrix-core Kalman kernel (csrc/kf_scan_bf32.hpp, MISSING = true;
DESIGN.md 4a''').  Two shapes at B = 16 384 trajectories and T = 250 steps, all five streams: a linear model (n = 32, m = 16,
K = 1) and Lorenz-96 with the even-state emission (n = 16, m = 8, K = 4).  The variants alternate over the rounds, each one
timed call on the same buffers:

  plain      the plain call on complete data (the one-wave matrix-core kernel)
  complete   the new route, nothing missing                (missing="nan" on the same data)
  gaps       the new route, 30 % of the entries missing    (independently per entry)
  tail       the same gaps, and the last fifth of the horizon not observed at all (a forecast: the update is skipped)
  anydim     the run-time-dimension kernel on the `gaps` inputs (options={"force_generic": 1}); linear shape only

Reported per shape: the median time of each variant, the plain call's own round-to-round spread ((max - min) / median), and the
ratios complete / plain, gaps / complete, tail / complete and anydim / gaps.

  python scripts/matrix_missing_probe.py [B] [T] [rounds]"""
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
T = int(sys.argv[2]) if len(sys.argv) > 2 else 250
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
    yt = yg.clone()
    yt[:, T - T // 5:] = float("nan")
    m0 = np.asarray(p.initial_mean, F32)
    init = torch.as_tensor((m0 + np.random.default_rng(n).normal(size=(B, K, n))).astype(F32), device="cuda")
    if kalman:
        init = init[:, 0]
    variants = [("plain", y, {}), ("complete", y, dict(missing="nan")), ("gaps", yg, dict(missing="nan")), ("tail", yt, dict(missing="nan"))]
    if kalman:
        variants.append(("anydim", yg, dict(missing="nan", options=GENERIC)))
    post = None
    for _, ys, kw in variants:                                   # warm-up: code objects, constants, the streams
        post, _ = run(p, ys[:, :8], K, init, kalman, None, **kw)
    post, _ = run(p, y, K, init, kalman, None)
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
    line = (f"  plain call's round-to-round spread {100 * spread:.2f} %;  complete / plain = {med['complete'] / med['plain']:.4f};  "
            f"gaps / complete = {med['gaps'] / med['complete']:.4f};  tail / complete = {med['tail'] / med['complete']:.4f}")
    if kalman:
        line += f";  anydim / gaps = {med['anydim'] / med['gaps']:.2f}"
    print(line, flush=True)
    del post, y, yg, yt
    torch.cuda.empty_cache()


shape_report("linear (32, 16)", linear_model(32, 16), 32, 16, 1, True)
shape_report("lorenz96 (16, 8)", lorenz96_model(16), 16, 8, 4, False)
