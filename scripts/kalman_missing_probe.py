"""Throughput of the Kalman filter's missing-observation route next to the plain filter at the headline shape.

n = 4, m = 2 (the constant-velocity model of bench.py), B = 65 536, T = 10 000, five streams, reference layout, output buffers
reused.  Three variants on the same emissions: ``kalman_filter``; ``kalman_filter(missing="nan")`` with nothing missing;
``kalman_filter(missing="nan")`` with 30 % of the entries NaN.  Each variant is warmed up, then the variants take turns for
--rounds rounds of --calls calls each, timed with device events; per variant the median, the lowest and the highest round in
timesteps/s, then the ratios of the medians to the plain filter's and the plain filter's own spread (highest / lowest round).
Usage: python scripts/kalman_missing_probe.py [--B 65536] [--T 10000] [--rounds 7] [--calls 3] [--out FILE]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bayesianfiltering_amd as bfa  # noqa: E402

F32 = np.float32


def cv_params(dt=0.5, q=1e-2, r=1e-1):
    nl = bfa.nonlinearities
    A = np.array([[1, dt, 0, 0], [0, 1, 0, 0], [0, 0, 1, dt], [0, 0, 0, 1]], F32)
    G = np.array([[0.5, 0], [1, 0], [0, 0.5], [0, 1]], F32)
    H = np.array([[1, 0, 0, 0], [0, 0, 1, 0]], F32)
    return bfa.ParamsNLSSM(np.zeros(4, F32), np.eye(4, dtype=F32), nl.linear_dynamics(A, G), np.zeros(2, F32), q * np.eye(2, dtype=F32),
                           nl.linear_emission(H, np.eye(2, dtype=F32)), np.zeros(2, F32), r * np.eye(2, dtype=F32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, T = args.B, args.T
    params = cv_params()
    gen = torch.Generator(device="cuda").manual_seed(0)
    y = torch.randn((B, T, 2), device="cuda", generator=gen)
    gaps = torch.where(torch.rand((B, T, 2), device="cuda", generator=gen) < 0.3, torch.full((), float("nan"), device="cuda"), y)
    init = torch.zeros((B, 4), device="cuda")
    st = {"post": None}

    def call(emissions, **kw):
        st["post"] = bfa.kalman_filter(params, emissions, initial_means=init, out=st["post"], **kw)

    variants = [("kalman_filter", lambda: call(y)),
                ("missing='nan', nothing missing", lambda: call(y, missing="nan")),
                ("missing='nan', 30 % missing", lambda: call(gaps, missing="nan"))]
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    finite = float(torch.isfinite(st["post"].means[:, 0, -1]).all(dim=1).float().mean())
    rates = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rates[name].append(B * T * args.calls / (e0.elapsed_time(e1) / 1e3))
    lines = [f"kalman_missing_probe: n=4 m=2 B={B} T={T} five streams, reference layout; {args.rounds} rounds x {args.calls} calls per "
             f"variant, variants alternating; device {torch.cuda.get_device_name(0)}; finite final means after the gapped run: {finite:.3f}"]
    med = {}
    for name, _ in variants:
        r = np.array(rates[name])
        med[name] = float(np.median(r))
        lines.append(f"{name:34s} median {med[name]:.4e} steps/s   lowest {r.min():.4e}   highest {r.max():.4e}   "
                     f"spread (highest / lowest) {r.max() / r.min():.4f}")
    base = variants[0][0]
    for name, _ in variants[1:]:
        lines.append(f"ratio to {base}: {name:34s} {med[name] / med[base]:.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
