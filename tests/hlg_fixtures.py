"""Inputs, fp64 oracle and tolerances of the histogram-loss (HL-Gauss) head problems shared by
tests/test_hlgauss_cpu.py (the fixture and tolerance checks that need no GPU) and tests/test_gpu_hlgauss.py
(the kernel)."""
import functools

import torch
from head_fixtures import split_planes

VMIN, VMAX = -10.0, 10.0
SIGMA = 0.75            # Runtime.hl_gauss_sigma_ratio's default
EPS = 1e-3              # Runtime.value_rescale_eps of the rescaled case
WSCALE = 2.0            # the sampler's factor handed to the IS statistic (a power of two: the division is exact)
SHAPES = [(64, 4, 51), (64, 18, 51), (64, 6, 21), (64, 3, 64), (5, 4, 51), (3, 3, 2)]
EDGE = (8, 4, 51)
FRAME_EDGE = (3, 2, 2)  # a block whose second sample is past the batch, fewer weight-row tasks (4) than waves
EDGE_CASES = ("rew_hi", "rew_lo", "terminal", "no_isw")
# tests/test_gpu_c51.py's seeds: generator seed 2, and 3 where seed 2 leaves a near-tie in the online argmax
# (FRAME_EDGE keeps seed 2: top-2 gap 1.18 in both input modes, fp64 on the CPU)
SEEDS = {(6, 21): 3, (3, 64): 3}

# Every head problem the GPU file runs: (B, A, N, split, case, sigma_ratio, rescale_eps)
PROBLEMS = ([(B, A, N, split, "plain", SIGMA, None) for (B, A, N) in SHAPES for split in (False, True)]
            + [(64, 4, 51, split, "plain", s, None) for s in (0.25, 2.0) for split in (False, True)]
            + [(*EDGE, False, case, SIGMA, None) for case in EDGE_CASES]
            + [(64, 4, 51, True, "plain", SIGMA, EPS)])

# Tolerances: tests/test_gpu_c51.py ``_compare``'s, except dhead's atol.  The target row inherits the fp32 error of
# y (about 2e-6 on |y| <= 10) times the Gaussian density per bin, which grows as sigma shrinks; C51's 1e-7 is not
# four times that.  Measured on the CPU over PROBLEMS, fp32 torch backend against the fp64 oracle: the largest
# absolute error of any dhead element, by (B, sigma_ratio) -- dhead carries grad_scale = 1 / B, so the small batches
# lead (tests/test_hlgauss_cpu.py re-measures, prints and bounds them):
STANDIN_DHEAD_ERR = {(64, 0.75): 4.5e-8, (64, 0.25): 5.6e-8, (64, 2.0): 2.7e-9, (8, 0.75): 1.1e-7, (5, 0.75): 2.0e-7,
                     (3, 0.75): 1.8e-8}
DHEAD_ATOL = 8e-7       # 4 x 2.0e-7, the largest of them
TOL = dict(td=(1e-4, 1e-4), loss=(1e-4, 1e-5), dH=(1e-2, 1e-6), dhead=(1e-4, DHEAD_ATOL), q=(1e-4, 1e-4),
           g=(1e-3, 1e-6))      # (rtol, atol); g: the four head weight gradients


@functools.lru_cache(maxsize=None)
def fixture(B, A, N, split=False):
    """Inputs (CPU) of one head problem, drawn as tests/test_gpu_c51.py draws them: Hon, Htg, online head,
    target head, act, rew, gam, isw."""
    g = torch.Generator().manual_seed(SEEDS.get((A, N), 2))
    Hon = torch.relu(torch.randn(2 * B, 1024, generator=g))
    Htg = torch.relu(torch.randn(B, 1024, generator=g))

    def P():
        return {"wv": torch.randn(N, 512, generator=g) * 0.05, "bv": torch.randn(N, generator=g),
                "wa": torch.randn(A * N, 512, generator=g) * 0.05, "ba": torch.randn(A * N, generator=g)}
    Pon, Ptg = P(), P()
    act = torch.randint(0, A, (B,), generator=g).to(torch.int32)
    rew = torch.randn(B, generator=g) * 3
    gam = torch.full((B,), 0.97)
    gam[::7] = 0.0
    isw = torch.rand(B, generator=g)
    if split:
        (Hon, Hon_lo), (Htg, Htg_lo) = split_planes(Hon), split_planes(Htg)
    else:
        Hon, Htg, Hon_lo, Htg_lo = Hon.to(torch.bfloat16), Htg.to(torch.bfloat16), None, None
    return dict(Hon=Hon, Htg=Htg, Hon_lo=Hon_lo, Htg_lo=Htg_lo, Pon=Pon, Ptg=Ptg, act=act, rew=rew, gam=gam, isw=isw)


def case_inputs(fx, case):
    B = fx["act"].shape[0]
    rew, gam, isw = fx["rew"], fx["gam"], fx["isw"]
    if case == "rew_hi":
        rew = torch.full((B,), 25.0)
    elif case == "rew_lo":
        rew = torch.full((B,), -25.0)
    elif case == "terminal":
        gam = torch.zeros(B)
    elif case == "no_isw":
        isw = None
    else:
        assert case == "plain", case
    return rew, gam, isw


def run_torch(B, A, N, split=False, case="plain", sigma=SIGMA, rescale_eps=None, dtype=torch.float64):
    """The torch backend in ``dtype`` on the joined activations of ``fixture(B, A, N, split)``: every output of
    the head and of the head weight gradient, the IS statistic and, in fp64, the oracle's own diagnostics."""
    from apex_dqn_amd.learner.rescale import rescale_target
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be = TorchBackend(dtype)
    fx = fixture(B, A, N, split)
    rew, gam, isw = case_inputs(fx, case)
    d = lambda t: t.to(dtype)                                            # noqa: E731
    join = lambda hi, lo: d(hi) if lo is None else d(hi.double() + lo.double())     # noqa: E731
    Hon, Htg = join(fx["Hon"], fx["Hon_lo"]), join(fx["Htg"], fx["Htg_lo"])
    Pon, Ptg = {k: d(v) for k, v in fx["Pon"].items()}, {k: d(v) for k, v in fx["Ptg"].items()}
    z = lambda *s: torch.zeros(*s, dtype=dtype)                          # noqa: E731
    td, loss, dH, dhead, q = z(B), z(B), z(B, 1024), z(B, (A + 1) * N), z(B, A)
    stat = (torch.full((1,), WSCALE), torch.full((1,), -1.0, dtype=torch.float64), torch.zeros((), dtype=torch.int64))
    be.hlg_head(Hon, Htg, Pon, Ptg, fx["act"], d(rew), d(gam), None if isw is None else d(isw), N, VMIN, VMAX, sigma,
                1.0 / B, td, loss, dH, dhead, q_out=q, isn=stat, rescale_eps=rescale_eps)
    gr = {k: torch.zeros_like(v) for k, v in Pon.items()}
    be.head_wgrad(Hon, dhead, gr)
    out = dict(td=td, loss=loss, dH=dH, dhead=dhead, q=q, g=gr, isn=float(stat[1]), count=int(stat[2]))
    if dtype == torch.float64:
        # diagnostics of the oracle alone: the top-2 gap of the online next-state q, the unclamped target, the
        # taken action's log-probabilities
        zs = VMIN + torch.arange(N, dtype=dtype) * ((VMAX - VMIN) / (N - 1))
        ar = torch.arange(B)
        qn = (be._c51_logp(Hon[B:2 * B], Pon, A, N, dtype).exp() * zs).sum(-1)
        top = qn.topk(2, dim=1).values
        qg = (be._c51_logp(Htg[:B], Ptg, A, N, dtype)[ar, qn.argmax(1)].exp() * zs).sum(-1)
        y0 = d(rew) + d(gam) * qg if rescale_eps is None else rescale_target(d(rew), d(gam), qg, rescale_eps)
        out.update(gap=float((top[:, 0] - top[:, 1]).min()), y0=y0,
                   lp=be._c51_logp(Hon[:B], Pon, A, N, dtype)[ar, fx["act"].long()])
    return out


@functools.lru_cache(maxsize=None)
def oracle(B, A, N, split=False, case="plain", sigma=SIGMA, rescale_eps=None):
    """fp64 CPU oracle (computed once per problem, shared, never modified)."""
    return run_torch(B, A, N, split, case, sigma, rescale_eps, torch.float64)


def _pairs(h, r):
    for k in ("td", "loss", "dH", "dhead", "q"):
        yield k, TOL[k], h[k], r[k]
    for k in ("wv", "bv", "wa", "ba"):
        yield "g_" + k, TOL["g"], h["g"][k], r["g"][k]


def compare(h, r):
    f = lambda t: t.float()                                              # noqa: E731
    for k, (rtol, atol), a, b in _pairs(h, r):
        torch.testing.assert_close(f(a), f(b), rtol=rtol, atol=atol, msg=lambda m, k=k: f"{k}: {m}")


def max_errors(h, r):
    """Largest error of every output in units of its tolerance (<= 1 passes) and, for dhead, in absolute terms."""
    out = {k: float(((a.double() - b.double()).abs() / (atol + rtol * b.double().abs())).max())
           for k, (rtol, atol), a, b in _pairs(h, r)}
    out["dhead_abs"] = float((h["dhead"].double() - r["dhead"].double()).abs().max())
    return out
