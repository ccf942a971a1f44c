"""Throughput of the particle filter's missing-observation route next to the plain filter at the bpf4096 shape.

N = 4096 particles, Lorenz-96 n = 16 observed through its even states (m = 8), B = 8192, T = 2000, summary output (the model
and the on-device data of bench.py --config bpf4096).  Three variants on the same emissions: ``bootstrap_particle_filter``;
``missing="nan"`` with nothing missing (isolates the per-step pattern test); ``missing="nan"`` with 30 % of the entries NaN (adds
the per-step factorisation of a partly observed step and the selects of the masked density).  Each variant is warmed up, then
the variants take turns for --rounds rounds of --calls calls each, timed with device events; per variant the median, the lowest
and the highest round in timesteps/s, then the ratios of the medians to the plain filter's and the plain filter's own spread.
Usage: python scripts/bpf_missing_probe.py [--B 8192] [--T 2000] [--rounds 5] [--calls 1] [--out FILE]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bayesianfiltering_amd as bfa  # noqa: E402

F32 = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, T, N, n, m = args.B, args.T, 4096, 16, 8
    nl = bfa.nonlinearities
    g = nl.pick_even(n)
    R = 0.5 * np.eye(m, dtype=F32)
    p = bfa.ParamsBPF(8 * np.ones(n, F32), np.eye(n, dtype=F32), nl.lorenz96(n), np.zeros(n, F32), 1e-2 * np.eye(n, dtype=F32), g,
                      np.zeros(m, F32), R, nl.gaussian_log_prob(g, R))
    from bayesianfiltering_amd import random as bfr
    _, y = bfa.NonlinearSSM(n, n, m, m).sample(bfa.ParamsNLSSM(*p[:8]), bfr.split(bfa.PRNGKey(4000), B), T)   # (bench.py's data)
    gen = torch.Generator(device="cuda").manual_seed(0)
    gaps = torch.where(torch.rand((B, T, m), device="cuda", generator=gen) < 0.3, torch.full((), float("nan"), device="cuda"), y)
    partly = float(((~torch.isnan(gaps)).any(dim=2) & torch.isnan(gaps).any(dim=2)).float().mean())
    key = np.array([0, 1], np.uint32)
    st = {}

    def call(emissions, **kw):
        st["out"] = bfa.bootstrap_particle_filter(p, emissions, N, key, output="summary", **kw)

    variants = [("bootstrap_particle_filter", lambda: call(y)),
                ("missing='nan', nothing missing", lambda: call(y, missing="nan")),
                ("missing='nan', 30 % missing", lambda: call(gaps, missing="nan"))]
    finite = {}
    for name, fn in variants:
        fn()
        torch.cuda.synchronize()
        finite[name] = float(torch.isfinite(st["out"]["mean"]).all(dim=(1, 2)).float().mean())
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
    lines = [f"bpf_missing_probe: N={N} n={n} m={m} B={B} T={T} summary output; {args.rounds} rounds x {args.calls} calls per variant, "
             f"variants alternating; device {torch.cuda.get_device_name(0)}; partly observed steps of the gapped series: {partly:.3f}; "
             f"trajectories with finite means: " + ", ".join(f"{finite[name]:.3f}" for name, _ in variants)]
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
