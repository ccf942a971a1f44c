"""Ad-hoc: what the missing-observation route of parallel_kalman_filter costs.  Model n = 4, m = 2 (the headline
constant-velocity model), all five streams, contiguous reference layout, default block, output buffers and workspace allocated
once (out= / workspace=).  Shapes B = 1, T = 10^6 and B = 64, T = 10^5.  Four variants on the same emissions, taking turns in
one process: the plain parallel filter; ``missing="nan"`` with nothing missing; ``missing="nan"`` with 30 % of the entries NaN;
the serial ``kalman_filter(missing="nan")`` on the same gapped emissions.  Per variant 2 warm-up rounds, then 7 timed rounds
with device events; the table shows the median and the spread (min ... max) in ms, trajectory-steps/s from the median, the
ratio of the median to the plain parallel filter's, and that filter's own run-to-run spread (max / min).

  python scripts/parallel_kalman_missing_probe.py [--out FILE]     # default profiles/parallel_kalman_missing_probe.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bayesianfiltering_amd as bfa
from tests import common as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "parallel_kalman_missing_probe.txt")
if "--out" in args:
    out_path = args[args.index("--out") + 1]
WARM, ROUNDS = 2, 7
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


a = cm.cv_model_arrays()
params = cm.product_params(a)
n, m = 4, 2


def emissions(B, T):
    """device observations: the model's own data for a short stretch, tiled in time (the filters' cost does not depend on the values)"""
    base = cm.simulate_batch(a, min(B, 64), min(T, 4096), seed=9)
    y = torch.as_tensor(base, device="cuda")
    return y.repeat((B + y.shape[0] - 1) // y.shape[0], (T + y.shape[1] - 1) // y.shape[1], 1)[:B, :T].contiguous()


def case(B, T):
    y = emissions(B, T)
    gen = torch.Generator(device="cuda").manual_seed(0)
    gaps = torch.where(torch.rand((B, T, m), device="cuda", generator=gen) < 0.3, torch.full((), float("nan"), device="cuda"), y)
    ws = torch.empty(bfa.parallel_kalman_workspace_bytes(n, m, B, T), dtype=torch.uint8, device="cuda")
    st = {"post": bfa.parallel_kalman_filter(params, y, workspace=ws)}

    def par(emis, **kw):
        st["post"] = bfa.parallel_kalman_filter(params, emis, out=st["post"], workspace=ws, **kw)

    def seq(emis):
        st["post"] = bfa.kalman_filter(params, emis, out=st["post"], missing="nan")

    variants = [("parallel_kalman_filter", lambda: par(y)),
                ("parallel, missing='nan', nothing missing", lambda: par(y, missing="nan")),
                ("parallel, missing='nan', 30 % missing", lambda: par(gaps, missing="nan")),
                ("kalman_filter(missing='nan'), 30 % missing", lambda: seq(gaps))]
    ms = {name: [] for name, _ in variants}
    for r in range(WARM + ROUNDS):
        for name, fn in variants:
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if r >= WARM:
                ms[name].append(s.elapsed_time(e))
        if r == 0:
            par(gaps, missing="nan")
            torch.cuda.synchronize()
            finite = bool(torch.isfinite(st["post"].means).all())
    base = float(np.median(ms[variants[0][0]]))
    for name, _ in variants:
        t = np.array(ms[name])
        med = float(np.median(t))
        say(f"B={B:4d} T={T:8d}  {name:44s} {med:10.3f} ms ({t.min():.3f} ... {t.max():.3f})  {B * T / med * 1e3:9.3e} steps/s"
            f"  x{med / base:7.3f} of plain   spread (max / min) {t.max() / t.min():.3f}")
    say(f"B={B:4d} T={T:8d}  every mean of the gapped parallel run finite: {finite}")
    del y, gaps, ws, st
    torch.cuda.empty_cache()


say(f"device: {torch.cuda.get_device_name(0)}; n={n}, m={m}, five streams, default block; {WARM} warm-up + {ROUNDS} timed rounds, "
    f"variants alternating; times are medians (min ... max)")
for B, T in ((1, 1_000_000), (64, 100_000)):
    case(B, T)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
