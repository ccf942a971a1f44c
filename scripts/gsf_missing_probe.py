"""Throughput of the Gaussian-sum filters' missing-observation route next to the plain filters.

Extended: the gsf32 shape of bench.py -- Lorenz-96 (as_written) n = 8, m = 4, K = 32, B = 16 384, T = 5 000, five streams in
T-chunks of 500 through the carry, output buffers reused, observations drawn from the model.  Unscented: the manoeuvring-target
model (4, 2, 2, 2) with K = 4, B = 16 384, T = 2 000.  Three variants on the same emissions: the plain filter; ``missing="nan"``
with nothing missing; ``missing="nan"`` with 30 % of the entries NaN.  Each variant is warmed up, then the variants take turns
for --rounds rounds of --calls calls each, timed with device events; per variant the median, the lowest and the highest round
in timesteps/s, then the ratios of the medians to the plain filter's and the plain filter's own spread (highest / lowest round).
Usage: python scripts/gsf_missing_probe.py [--B 16384] [--T 5000] [--rounds 5] [--calls 1] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bayesianfiltering_amd as bfa  # noqa: E402
from bench import simulate_on_device  # noqa: E402

F32 = np.float32


def with_gaps(y, gen):
    return torch.where(torch.rand(y.shape, device=y.device, generator=gen) < 0.3, torch.full((), float("nan"), device=y.device), y)


def take_turns(variants, units, rounds, calls):
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rates[name].append(units * calls / (e0.elapsed_time(e1) / 1e3))
    lines, med = [], {}
    for name, _ in variants:
        r = np.array(rates[name])
        med[name] = float(np.median(r))
        lines.append(f"{name:34s} median {med[name]:.4e} steps/s   lowest {r.min():.4e}   highest {r.max():.4e}   "
                     f"spread (highest / lowest) {r.max() / r.min():.4f}")
    base = variants[0][0]
    for name, _ in variants[1:]:
        lines.append(f"ratio to {base}: {name:34s} {med[name] / med[base]:.4f}")
    return lines


def extended(B, T, chunk, rounds, calls):
    nl = bfa.nonlinearities
    K, n = 32, 8
    p = bfa.ParamsNLSSM(8 * np.ones(8, F32), np.eye(8, dtype=F32), nl.lorenz96(8, mode="as_written"), np.zeros(8, F32),
                        1e-2 * np.eye(8, dtype=F32), nl.pick_even(8), np.zeros(4, F32), 1e-1 * np.eye(4, dtype=F32))
    y = simulate_on_device(p, (8, 8, 4, 4), B, T, seed=2000, first=0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    gaps = with_gaps(y, gen)
    init = 8.0 + torch.randn((B, K, n), device="cuda", generator=gen)
    st = {"post": None, "carry": None}

    def call(emissions, **kw):
        carry = None
        for t0 in range(0, T, chunk):
            yc = emissions[:, t0:t0 + chunk]
            reuse = st["post"] if (st["post"] is not None and st["post"].weights.shape[2] == yc.shape[1]) else None
            st["post"], carry = bfa.gaussian_sum_filter(p, yc, K, 1, initial_means=init, carry=carry, out=reuse, return_carry=True, **kw)
        st["carry"] = carry

    variants = [("gaussian_sum_filter", lambda: call(y)),
                ("missing='nan', nothing missing", lambda: call(y, missing="nan")),
                ("missing='nan', 30 % missing", lambda: call(gaps, missing="nan"))]
    lines = take_turns(variants, B * T, rounds, calls)
    finite = float(torch.isfinite(st["carry"].means).all(dim=(1, 2)).float().mean())
    head = (f"gsf_missing_probe, extended: Lorenz-96[as_written] n=8 m=4 K={K} B={B} T={T}, five streams in chunks of {chunk}; "
            f"{rounds} rounds x {calls} calls per variant, variants alternating; device {torch.cuda.get_device_name(0)}; "
            f"finite final means after the gapped run: {finite:.3f}")
    st.clear()
    return [head] + lines


def unscented(B, T, rounds, calls):
    nl = bfa.nonlinearities
    K = 4
    mu0 = np.array([2.0, 0.3, 3.0, -0.2], F32)
    p = bfa.ParamsNLSSM(mu0, np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32), nl.maneuver_bot(), np.zeros(2, F32), 1e-3 * np.eye(2, dtype=F32),
                        nl.bearing_range(), np.zeros(2, F32), np.diag([1e-3, 1e-2]).astype(F32))
    up = bfa.ParamsUKF(1.0, 0.0, 0.0)
    y = simulate_on_device(p, (4, 2, 2, 2), B, T, seed=2100, first=0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    gaps = with_gaps(y, gen)
    init = torch.as_tensor(mu0, device="cuda") + 0.05 * torch.randn((B, K, 4), device="cuda", generator=gen)
    st = {"post": None}

    def call(emissions, **kw):
        st["post"] = bfa.unscented_gaussian_sum_filter(p, up, emissions, K, 1, initial_means=init, out=st["post"], **kw)

    variants = [("unscented_gaussian_sum_filter", lambda: call(y)),
                ("missing='nan', nothing missing", lambda: call(y, missing="nan")),
                ("missing='nan', 30 % missing", lambda: call(gaps, missing="nan"))]
    lines = take_turns(variants, B * T, rounds, calls)
    finite = float(torch.isfinite(st["post"].means[:, :, -1]).all(dim=(1, 2)).float().mean())
    head = (f"gsf_missing_probe, unscented: manoeuvring target + bearing / range (4, 2, 2, 2) K={K} B={B} T={T}, five streams; "
            f"{rounds} rounds x {calls} calls per variant, variants alternating; finite final means after the gapped run: {finite:.3f}")
    return [head] + lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16384)
    ap.add_argument("--T", type=int, default=5000)
    ap.add_argument("--chunk", type=int, default=500)
    ap.add_argument("--uT", type=int, default=2000, help="horizon of the unscented run")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = extended(args.B, args.T, args.chunk, args.rounds, args.calls)
    torch.cuda.empty_cache()
    lines += unscented(args.B, args.uT, args.rounds, args.calls)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
