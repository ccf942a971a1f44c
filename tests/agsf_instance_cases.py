"""The case table of the every-instance sweep of the augmented Gaussian-sum register kernels (csrc/agsf_scan.hpp, dispatched by
agsf_scan.hip / agsf_ukf.hip over a table of instances times launch geometries), shared by test_agsf_instances_cpu.py (which
checks, without a GPU, that each case is a meaningful comparison and that the table reaches every compiled kernel) and
test_agsf_instances_gpu.py (which runs the cases on the device).  Every oracle run is computed once per process and handed out
read-only.

ROWS: one model per compiled instance -- a nonlinear registry model where there is one at that shape (analytic Jacobians, the
state-dependent noise gain of the multiplicative-noise emission), and a linear twin with a non-square noise map and noise biases
wherever the shape allows one.  TIERS: one tree per launch geometry, no leaf count a power of two; the multi-wave launches round
their carried records to (N0 + 3) & ~3 and N0 = 5, 6 and 10 are no multiples of 4.

CASES: name -> dict(row, tier, nc, T, B, variant, uparams, refs, seed, spread); ``refs`` are the trajectories of the batch that are
compared with the oracle."""
import functools

import numpy as np

from oracle import gaussfilt_oracle as go, models as om, threefry as otf
from tests import common as cm
from tests.agsf_generic_cases import optimal_key

F32 = np.float32
UP = (1.0, 0.0, 0.0)


def _row(kind, inst, model, spread=1.0, **kw):
    return dict(kind=kind, inst=tuple(inst), model=model, spread=spread, **kw)


# kind "ekf": instance (n, m); kind "ukf": instance (n, dq, m, dr).  ``spread``: standard deviation of the initial means around m0
# (0.05 for the manoeuvring target, as in tests/test_agsf_gpu.py: its bearing is undefined at the origin).
ROWS = {
    "e11-sine": _row("ekf", (1, 1), "sine_quad"),
    "e11-growth": _row("ekf", (1, 1), "growth_quad"),
    "e21-sine": _row("ekf", (2, 1), "sine_quad"),
    "e21-lin": _row("ekf", (2, 1), "linear", dq=1, dr=1),
    "e22-sv": _row("ekf", (2, 2), "stochvol"),
    "e22-lin": _row("ekf", (2, 2), "linear", dq=1, dr=2),
    "e31-l63": _row("ekf", (3, 1), "l63_quad"),
    "e33-l63": _row("ekf", (3, 3), "l63_linear"),
    "e33-lin": _row("ekf", (3, 3), "linear", dq=3, dr=2),
    "e41-bot": _row("ekf", (4, 1), "bot_bearing", spread=0.05),
    "e42-bot": _row("ekf", (4, 2), "bot_bearing_range", spread=0.05),
    "e42-lin": _row("ekf", (4, 2), "linear", dq=3, dr=1),
    "e84-l96": _row("ekf", (8, 4), "l96"),
    # (8, 4) linear at (4, 3, 5): initial means of unit spread left 1.17 distinct drawn leaves per step (the first observation
    # picks one component and the tree never recovers) -- a spread of 0.1 keeps the components comparable
    "e84-lin": _row("ekf", (8, 4), "linear", dq=5, dr=3, spread=0.1),
    "u1111-sine": _row("ukf", (1, 1, 1, 1), "sine_quad"),
    "u3311-l63": _row("ukf", (3, 3, 1, 1), "l63_quad"),
    "u4211-bot": _row("ukf", (4, 2, 1, 1), "bot_bearing", spread=0.05),
    "u4222-bot": _row("ukf", (4, 2, 2, 2), "bot_bearing_range", spread=0.05),
    "u4422-lin": _row("ukf", (4, 4, 2, 2), "linear", dq=4, dr=2),
}

# tier -> (tree, B, T, trajectories compared with the oracle).  With one wave per trajectory a 256-thread workgroup holds 256 / MP
# trajectories: G1a is two full workgroups and a tail of 5 (trajectory 36 is the last of the tail), G1b one full workgroup and a
# tail of 3.  G2 is the reference's own test tree, G8 the tree of BOT_Experiment_script.py.
TIERS = {
    "G1a": ((3, 2, 2), 37, 8, (0, 20, 36)),
    "G1b": ((4, 3, 5), 7, 8, (0, 6)),
    "G2": ((5, 5, 5), 2, 6, (0, 1)),
    "G4": ((6, 5, 7), 2, 6, (0, 1)),
    "G8": ((100, 2, 2), 2, 6, (0, 1)),
    "G16": ((10, 10, 10), 2, 6, (0, 1)),
}
ONE_WAVE = ("G1a", "G1b")

# Replacements under the meaningful-comparison conditions of test_agsf_instances_cpu.py: (row, tier, variant) -> what differs from
# the default seed 0 / the row's spread / the tier's T.  Each entry says which condition the default missed.
# Optimal resampling (variant 2) needed most of them.  While no leaf weight reaches the threshold every output is drawn through the
# SORTED order of the weights and is emitted with weight 1 / N0: hundreds of leaves of a one- or two-dimensional model hold pairs
# within 1e-4 of each other (no margin), and the emitted weights are all equal (not the point of the variant).  A LARGER spread of
# the initial means lets the first observation single out a few leaves, and a shorter T ends the series before the tree has
# contracted again (T = 2 still carries the unequal weights into a second step once).
OVERRIDES = {
    ("e11-sine", "G1a", 2): dict(seed=2),      # emitted weights all 1 / N0
    ("e11-sine", "G1b", 2): dict(seed=45),      # emitted weights all 1 / N0
    ("e11-sine", "G2", 2): dict(seed=5, T=3),      # emitted weights all 1 / N0
    ("e11-sine", "G4", 0): dict(seed=1),      # a draw without margin (step 4)
    ("e11-sine", "G4", 2): dict(seed=5, spread=8.0, T=2),      # emitted weights all 1 / N0
    ("e11-sine", "G8", 2): dict(seed=238, T=2),      # a draw without margin (step 0)
    ("e11-sine", "G16", 2): dict(seed=187, spread=4.0, T=2),      # emitted weights all 1 / N0
    ("e11-growth", "G1b", 2): dict(seed=9, spread=2.0),      # a draw without margin (step 3)
    ("e11-growth", "G2", 2): dict(seed=0, T=3),      # a draw without margin (step 5)
    ("e11-growth", "G4", 2): dict(seed=2, spread=128.0, T=3),      # a draw without margin (step 3)
    ("e11-growth", "G8", 2): dict(seed=8, spread=128.0, T=2),      # a draw without margin (step 0)
    ("e11-growth", "G16", 0): dict(seed=1),      # a draw without margin (step 1)
    ("e11-growth", "G16", 2): dict(seed=15, spread=128.0, T=3),      # a draw without margin (step 0)
    ("e21-sine", "G1b", 2): dict(seed=55, spread=2.0),      # emitted weights all 1 / N0
    ("e21-sine", "G2", 2): dict(seed=136, T=3),      # emitted weights all 1 / N0
    ("e21-sine", "G4", 2): dict(seed=160, T=2),      # emitted weights all 1 / N0
    ("e21-sine", "G8", 0): dict(seed=7),      # a draw without margin (step 1)
    ("e21-sine", "G8", 2): dict(seed=128, T=2),      # a draw without margin (step 0)
    ("e21-sine", "G16", 2): dict(seed=179, spread=64.0, T=2),      # emitted weights all 1 / N0
    ("e21-lin", "G1b", 2): dict(seed=10, spread=16.0),      # a draw without margin (step 6)
    ("e21-lin", "G2", 2): dict(seed=4, spread=16.0),      # a draw without margin (step 4)
    ("e21-lin", "G4", 2): dict(seed=0, spread=16.0, T=4),      # a draw without margin (step 1)
    ("e21-lin", "G8", 2): dict(seed=12, spread=10.0, T=2),      # a draw without margin (step 0)
    ("e21-lin", "G16", 2): dict(seed=0, spread=80.0, T=3),      # a draw without margin (step 1)
    ("e22-sv", "G1a", 2): dict(seed=6, spread=4.0),      # emitted weights all 1 / N0
    ("e22-sv", "G1b", 2): dict(seed=5, spread=32.0, T=3),      # a draw without margin (step 3)
    ("e22-sv", "G2", 2): dict(seed=7, spread=32.0, T=3),      # emitted weights all 1 / N0
    ("e22-sv", "G4", 2): dict(seed=2, spread=32.0, T=3),      # a draw without margin (step 0)
    ("e22-sv", "G8", 0): dict(seed=3),      # a draw without margin (step 5)
    ("e22-sv", "G8", 2): dict(seed=4, spread=20.0, T=2),      # a draw without margin (step 0)
    ("e22-sv", "G16", 2): dict(seed=118, spread=40.0, T=3),      # a draw without margin (step 0)
    ("e22-lin", "G4", 2): dict(seed=2),      # a draw without margin (step 4)
    ("e22-lin", "G8", 2): dict(seed=15),      # a draw without margin (step 5)
    ("e22-lin", "G16", 2): dict(seed=15, T=4),      # a draw without margin (step 2)
    ("e31-l63", "G1a", 2): dict(seed=1, spread=16.0),      # a draw without margin (step 3)
    ("e31-l63", "G1b", 2): dict(seed=1, spread=16.0),      # a draw without margin (step 3)
    ("e31-l63", "G2", 2): dict(seed=0, spread=32.0, T=4),      # a draw without margin (step 2)
    ("e31-l63", "G4", 2): dict(seed=1, spread=16.0, T=3),      # a draw without margin (step 1)
    ("e31-l63", "G8", 2): dict(seed=85, spread=20.0, T=3),      # a draw without margin (step 0)
    ("e31-l63", "G16", 2): dict(seed=4, spread=20.0),      # a draw without margin (step 0)
    ("e33-l63", "G1a", 1): dict(seed=1),      # a degenerate tree (1.25 distinct leaves per step)
    ("e33-l63", "G4", 0): dict(seed=1),      # a draw without margin (step 5)
    ("e33-l63", "G8", 0): dict(seed=1),      # a draw without margin (step 5)
    ("e33-l63", "G8", 2): dict(seed=3),      # a draw without margin (step 4)
    ("e33-l63", "G16", 2): dict(seed=36),      # a draw without margin (step 4)
    ("e33-lin", "G1a", 0): dict(seed=8),      # a degenerate tree (1.12 distinct leaves per step)
    ("e33-lin", "G1a", 1): dict(seed=17),      # a degenerate tree (1.25 distinct leaves per step)
    ("e33-lin", "G1a", 2): dict(seed=25),      # best leaf at |log-likelihood| 4557
    ("e33-lin", "G1b", 2): dict(seed=2),      # best leaf at |log-likelihood| 1057
    ("e33-lin", "G2", 0): dict(seed=1),      # a degenerate tree (1.33 distinct leaves per step)
    ("e33-lin", "G4", 2): dict(seed=7),      # best leaf at |log-likelihood| 2039
    ("e33-lin", "G8", 0): dict(seed=2),      # a draw without margin (step 0)
    ("e33-lin", "G8", 2): dict(seed=4),      # a draw without margin (step 0)
    ("e33-lin", "G16", 2): dict(seed=2, spread=4.0),      # a draw without margin (step 4)
    ("e41-bot", "G1b", 2): dict(seed=3),      # a draw without margin (step 3)
    ("e41-bot", "G2", 2): dict(seed=6, spread=0.8),      # emitted weights all 1 / N0
    ("e41-bot", "G4", 2): dict(seed=87, spread=0.1, T=3),      # a draw without margin (step 5)
    ("e41-bot", "G8", 0): dict(seed=2),      # a draw without margin (step 0)
    ("e41-bot", "G8", 2): dict(seed=2, spread=16.0, T=3),      # a draw without margin (step 1)
    ("e41-bot", "G16", 2): dict(seed=34, spread=3.2, T=3),      # a draw without margin (step 1)
    ("e42-bot", "G1b", 2): dict(seed=3),      # a draw without margin (step 7)
    ("e42-bot", "G2", 2): dict(seed=1, spread=0.2),      # emitted weights all 1 / N0
    ("e42-bot", "G4", 2): dict(seed=1, spread=0.2),      # a draw without margin (step 5)
    ("e42-bot", "G8", 0): dict(seed=1),      # a draw without margin (step 3)
    ("e42-bot", "G8", 2): dict(seed=98, T=3),      # a draw without margin (step 3)
    ("e42-bot", "G16", 2): dict(seed=14, spread=0.8, T=3),      # a draw without margin (step 2)
    ("e42-lin", "G1a", 0): dict(seed=18),      # a degenerate tree (1.12 distinct leaves per step)
    ("e42-lin", "G1a", 1): dict(seed=18),      # a degenerate tree (1.00 distinct leaves per step)
    ("e42-lin", "G1a", 2): dict(seed=72),      # best leaf at |log-likelihood| 2262
    ("e42-lin", "G1b", 2): dict(seed=3),      # best leaf at |log-likelihood| 982
    ("e42-lin", "G8", 0): dict(seed=3),      # a draw without margin (step 4)
    ("e42-lin", "G8", 2): dict(seed=3),      # a draw without margin (step 2)
    ("e84-l96", "G1a", 2): dict(seed=1),      # a draw without margin (step 1)
    ("e84-lin", "G1a", 0): dict(seed=1, spread=0.02),      # a degenerate tree (1.38 distinct leaves per step)
    ("e84-lin", "G1a", 1): dict(seed=14, spread=0.5, T=6),      # a degenerate tree (1.25 distinct leaves per step)
    ("e84-lin", "G1a", 2): dict(seed=13),      # best leaf at |log-likelihood| 633
    ("e84-lin", "G1b", 0): dict(seed=1),      # a degenerate tree (1.12 distinct leaves per step)
    ("u4211-bot", "G8", 0): dict(seed=2),      # a draw without margin (step 2)
    ("u4222-bot", "G8", 0): dict(seed=1),      # a draw without margin (step 5)
}


def geometry(nc):
    """(MP, nw) as prepare_agsf (csrc/agsf_geom.hpp) computes them from the tree."""
    leaves = int(np.prod(nc))
    MP = 1
    while MP < leaves:
        MP <<= 1
    return MP, (1 if MP <= 64 else MP // 64)


def _cases():
    out = {}
    for rname, r in ROWS.items():
        for tname, (nc, B, T, refs) in TIERS.items():
            if r["inst"][0] > 4 and tname not in ONE_WAVE:     # the multi-wave geometries exist for n <= 4 only
                continue
            variants = [0] + ([2] if r["kind"] == "ekf" else []) + ([1] if tname == "G1a" else [])
            for v in variants:
                o = OVERRIDES.get((rname, tname, v), {})
                name = f"{rname}-{tname}-v{v}"
                out[name] = dict(name=name, row=rname, tier=tname, nc=nc, B=B, T=o.get("T", T), refs=refs, variant=v,
                                 uparams=UP if r["kind"] == "ukf" else None, seed=o.get("seed", 0),
                                 spread=o.get("spread", r["spread"]), n=r["inst"][0])
    return out


CASES = _cases()


def kernel_of(row, nc):
    """(node kind, instance, waves per trajectory): the compiled kernel a call with this row's model and this tree launches."""
    r = ROWS[row]
    return r["kind"], r["inst"], geometry(nc)[1]


@functools.lru_cache(maxsize=None)
def model_arrays(row):
    """Everything both sides need to build the model of a row, as plain arrays."""
    r = ROWS[row]
    kind = r["model"]
    n = r["inst"][0]
    rng = np.random.default_rng(23)
    eye = lambda d, s=1.0: (s * np.eye(d)).astype(F32)
    if kind == "linear":
        m = r["inst"][1] if r["kind"] == "ekf" else r["inst"][2]
        d = cm.random_stable_lgssm(n, m, seed=10 * n + m, dq=r["dq"], dr=r["dr"], bias=True)
    elif kind == "sine_quad":       # f1 / g1 of Experiment_TSP_2023.ipynb at w0 = 1.5 (tests/test_ugsf_gpu.py), with noise biases
        d = dict(m0=np.zeros(n, F32), P0=eye(n), q0=np.full(n, 0.05, F32), Q=eye(n, 0.1), r0=np.array([-0.1], F32), R=eye(1, 0.02))
    elif kind == "growth_quad":     # f3 of the same notebook with the quadratic emission x^2 / 20; the input is the model's forcing
        d = dict(m0=np.zeros(1, F32), P0=eye(1), q0=np.array([0.05], F32), Q=eye(1), r0=np.array([-0.1], F32), R=eye(1))
    elif kind == "stochvol":        # the model of tests/test_ugsf_gpu.py::test_stochastic_volatility_non_additive_noise
        d = dict(m0=np.zeros(2, F32), P0=eye(2), q0=np.zeros(2, F32), Q=eye(2, 0.5), r0=np.array([0.1, -0.2], F32), R=eye(2, 0.1),
                 Phi=eye(2, 0.8))
    elif kind == "l63_quad":        # tests/test_ugsf_gpu.py::test_lorenz63_quadratic_and_scalar_models
        d = dict(m0=np.array([0.0, 1.0, 1.05], F32), P0=eye(3), q0=np.zeros(3, F32), Q=eye(3, 0.1), r0=np.zeros(1, F32), R=eye(1))
    elif kind == "l63_linear":      # a dense emission whose two noises enter three observations
        Lr = 0.3 * rng.normal(size=(2, 2))
        d = dict(m0=np.array([0.0, 1.0, 1.05], F32), P0=eye(3), q0=np.array([0.02, -0.01, 0.03], F32), Q=eye(3, 0.1),
                 r0=np.array([0.1, -0.2], F32), R=(Lr @ Lr.T + 0.1 * np.eye(2)).astype(F32),
                 H=(rng.normal(size=(3, 3)) / np.sqrt(3)).astype(F32), D=(np.eye(3, 2) + 0.1 * rng.normal(size=(3, 2))).astype(F32))
    elif kind == "bot_bearing":     # tests/test_reference_smoke_gpu.py with R = 1e-2
        d = dict(m0=np.ones(4, F32), P0=np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32), q0=np.zeros(2, F32), Q=eye(2),
                 r0=np.zeros(1, F32), R=eye(1, 1e-2))
    elif kind == "bot_bearing_range":   # tests/test_agsf_gpu.py, with noise biases
        d = dict(m0=np.array([2.0, 0.3, 3.0, -0.2], F32), P0=np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32),
                 q0=np.array([0.01, -0.02], F32), Q=eye(2, 1e-3), r0=np.array([0.005, -0.01], F32), R=np.diag([1e-3, 1e-2]).astype(F32))
    elif kind == "l96":             # tests/test_agsf_gpu.py::test_lorenz96_and_errors
        d = dict(m0=np.zeros(n, F32), P0=eye(n), q0=np.zeros(n, F32), Q=eye(n, 1e-2), r0=np.zeros(n // 2, F32), R=eye(n // 2, 1e-1))
    else:
        raise KeyError(kind)
    return dict(d, kind=kind)


def _functions(row, lib, linear_dyn, linear_emi):
    """(f, h) of a nonlinear row from the oracle's model zoo or from the package's registry (the same constructor names but for case)."""
    d = model_arrays(row)
    kind, n = d["kind"], ROWS[row]["inst"][0]
    pick = lambda a, b: getattr(lib, a) if hasattr(lib, a) else getattr(lib, b)
    sine, quad, growth = pick("Sine", "sine"), pick("Quadratic", "quadratic"), pick("Growth", "growth")
    l63, l96, even = pick("Lorenz63", "lorenz63"), pick("Lorenz96", "lorenz96"), pick("PickEven", "pick_even")
    bot, bearing, brange, sv = pick("ManeuverBOT", "maneuver_bot"), pick("Bearing", "bearing"), pick("BearingRange", "bearing_range"), pick("StochVol", "stoch_vol")
    return {"sine_quad": lambda: (sine(n, 1.5), quad(n, 0.5)),
            "growth_quad": lambda: (growth(), quad(1, 0.05)),
            "stochvol": lambda: (linear_dyn(d["Phi"]), sv(2)),
            "l63_quad": lambda: (l63(), quad(3, 0.05)),
            "l63_linear": lambda: (l63(), linear_emi(d["H"], d["D"])),
            "bot_bearing": lambda: (bot(), bearing()),
            "bot_bearing_range": lambda: (bot(), brange()),
            "l96": lambda: (l96(n), even(n))}[kind]()


def oracle_model(row):
    d = model_arrays(row)
    if d["kind"] == "linear":
        return cm.oracle_params(d)
    f, h = _functions(row, om, om.Linear, om.Linear)
    return go.ParamsNLSSM(d["m0"], d["P0"], f, d["q0"], d["Q"], h, d["r0"], d["R"])


def product_model(row):
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    d = model_arrays(row)
    if d["kind"] == "linear":
        return cm.product_params(d)
    f, h = _functions(row, nl, nl.linear_dynamics, nl.linear_emission)
    return bfa.ParamsNLSSM(d["m0"], d["P0"], f, d["q0"], d["Q"], h, d["r0"], d["R"])


def inputs_of(row, T):
    """(T,) inputs of a row or None: the growth model's forcing 8 cos(1.2 t), the volatility switch 0 -> 1 halfway, the
    manoeuvre indicator 1 / 0 / 2 by thirds."""
    kind = ROWS[row]["model"]
    if kind == "growth_quad":
        return (8.0 * np.cos(1.2 * np.arange(T))).astype(F32)
    if kind == "stochvol":
        return np.array([0] * (T // 2) + [1] * (T - T // 2), F32)
    if kind.startswith("bot"):
        a = T // 3
        return np.array([1] * a + [0] * a + [2] * (T - 2 * a), F32)
    return None


def inputs(name):
    c = CASES[name]
    return inputs_of(c["row"], c["T"])


@functools.lru_cache(maxsize=None)
def _data(row, N0, T, B, seed, spread):
    d = model_arrays(row)
    n = d["m0"].size
    u = inputs_of(row, T)
    po = oracle_model(row)
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(2 + b + 100 * seed), T, None if u is None else u.reshape(T, 1))[1] for b in range(B)])
    init = np.stack([(d["m0"] + spread * np.random.default_rng(1 + b + 100 * seed).normal(size=(N0, n))).astype(F32) for b in range(B)])
    ys.setflags(write=False)
    init.setflags(write=False)
    return ys, init


def data(name):
    """(emissions (B, T, m), initial means (B, N0, n)) of a case: trajectory b from sample_ssm(PRNGKey(2 + b)) and default_rng(1 + b),
    as agsf_generic_cases.data draws them (a replacement seed s shifts both by 100 s)."""
    c = CASES[name]
    return _data(c["row"], c["nc"][0], c["T"], c["B"], c["seed"], c["spread"])


def run_oracle(name, b):
    """The oracle on trajectory b of the case.  aux also gets 'best_loglik' (T,): the largest leaf log-likelihood of every step, as
    the oracle hands it to its weight update."""
    c = CASES[name]
    ys, init = data(name)
    u = inputs(name)
    best, keep = [], go.reweight

    def recording(lls, weights):
        l = np.asarray(lls, dtype=np.float64)
        best.append(float(np.max(l[np.isfinite(l)])) if np.isfinite(l).any() else np.nan)
        return keep(lls, weights)

    go.reweight = recording
    try:
        post, aux = go.speedy_augmented_gaussian_sum_filter(oracle_model(c["row"]), ys[b], c["nc"], None, 1, (0.1, 0.1),
                                                            None if u is None else u.reshape(c["T"], 1), initial_means=init[b], debug=True,
                                                            variant=c["variant"], uparams=None if c["uparams"] is None else go.ParamsUKF(*c["uparams"]))
    finally:
        go.reweight = keep
    aux["best_loglik"] = np.array(best)
    return post, aux


@functools.lru_cache(maxsize=None)
def reference(name, b):
    """(posterior, aux) of the oracle on trajectory b of the case; aux holds pre_weights and leaf_indices per step."""
    post, aux = run_oracle(name, b)
    for v in list(post) + list(aux.values()):
        if v is not None:
            v.setflags(write=False)
    return post, aux


def draw(name, w):
    """The leaves one step draws from the leaf weights w, by the case's resampling rule."""
    c = CASES[name]
    N0 = c["nc"][0]
    w = np.asarray(w, dtype=F32)
    if c["variant"] == 2:
        return np.asarray(go.optimal_resampling(w, N0, optimal_key())[0], dtype=np.int32)
    idx = otf.choice_indices(otf.cumsum_assoc(w), otf.uniform(otf.PRNGKey(0), N0))
    return np.minimum(idx, w.size - 1).astype(np.int32)


def margin_patterns(name):
    """The sign patterns of the margin condition: alternating (both signs), as test_agsf_generic_cpu.py has them; for optimal
    resampling one pattern per bit of the leaf index (both signs; bit 0 is the alternating one).  Its draw goes through the sorted
    order of the weights, and the alternating pattern scales two leaves of equal parity alike: a near-tie between them went
    unseen, and the device drew another leaf than the oracle (linear (4, 2) row at (100, 2, 2): weights 1.15493e-16 and
    1.15491e-16 of leaves 299 and 133).  Two different leaves differ in some bit, so some pattern pulls every pair apart."""
    M = int(np.prod(CASES[name]["nc"]))
    bits = range(max(1, (M - 1).bit_length())) if CASES[name]["variant"] == 2 else (0,)
    out = []
    for k in bits:
        signs = np.where((np.arange(M) >> k) % 2 == 0, 1.0, -1.0)
        out += [signs, -signs]
    return out


def oracle_leaf_indices(name, b):
    """Per-step drawn leaves recomputed from the oracle's leaf weights, or the oracle's own record for optimal resampling."""
    _, aux = reference(name, b)
    if CASES[name]["variant"] == 2:
        return np.asarray(aux["leaf_indices"], dtype=np.int32)
    return np.stack([draw(name, w) for w in aux["pre_weights"]])


def linear_covariances_f64(row, nc, leaf, covs, P0):
    """For a linear row the covariance of a leaf does not depend on the drawn points.  Teacher-forced in float64 from a run's own
    covariances ``covs`` (N0, T, n, n) and drawn leaves ``leaf`` (T, N0):  i0 = leaf // (N1 N2),
    Lam = a1 (A (a0 P[t-1, i0]) A^T + G Q G^T),  S = H Lam H^T + D R D^T,  K = Lam H^T (S + 1e-6)^-1 (the jitter on every entry,
    as psd_solve adds it),  P[t, j] = Lam - K S K^T.  Returns (N0, T, n, n)."""
    d = {k: np.asarray(v, dtype=np.float64) for k, v in model_arrays(row).items() if k != "kind"}
    a0 = a1 = float(F32(0.1))
    N0, N1, N2 = nc
    T = leaf.shape[0]
    GQG, DRD = d["G"] @ d["Q"] @ d["G"].T, d["D"] @ d["R"] @ d["D"].T
    out = np.empty((N0, T) + d["P0"].shape)
    for t in range(T):
        for j in range(N0):
            i0 = int(leaf[t, j]) // (N1 * N2)
            prev = np.asarray(P0, dtype=np.float64) if t == 0 else np.asarray(covs[i0, t - 1], dtype=np.float64)
            Lam = a1 * (d["A"] @ (a0 * prev) @ d["A"].T + GQG)
            S = d["H"] @ Lam @ d["H"].T + DRD
            K = np.linalg.solve(S + 1e-6, d["H"] @ Lam).T
            out[j, t] = Lam - K @ S @ K.T
    return out
