"""Inputs and fp64 oracle of the implicit quantile head problems shared by tests/test_iqn_cpu.py
(the tolerance and fixture checks that need no GPU) and tests/test_gpu_iqn.py (the kernels)."""
import functools

import torch
from head_fixtures import split_planes

KAPPA = 1.0
SEED = 12345            # Runtime.seed of the head problems
CTR, BASE = 9, 2        # draw counter and base word: update index u = 7
SHAPES = [(64, 4, 8), (64, 18, 64), (64, 6, 21), (64, 2, 2), (5, 4, 8), (13, 4, 8)]
WSCALE = 2.0            # the sampler's factor handed to the IS statistic (a power of two: the division is exact)
KINK = 1e-5             # |pre| below this in the fp64 oracle: a ReLU-mask flip is a one-term difference


def seed_q():
    from apex_dqn_amd.learner.iqn import iqn_seed
    return iqn_seed(SEED)


@functools.lru_cache(maxsize=None)
def fixture(B, A, split=False):
    """Inputs (CPU) of one head problem, drawn as tests/test_gpu_qr.py draws them (generator seed 2,
    the order Hon, Htg, online head, target head, act, rew, gam, isw) with the scalar head's
    shapes, then the two embeddings: We ~ N(0, 1/64) and be ~ N(0, 0.1) (variances)."""
    g = torch.Generator().manual_seed(2)
    Hon = torch.relu(torch.randn(2 * B, 1024, generator=g))
    Htg = torch.relu(torch.randn(B, 1024, generator=g))

    def P():
        return {"wv": torch.randn(1, 512, generator=g) * 0.05, "bv": torch.randn(1, generator=g),
                "wa": torch.randn(A, 512, generator=g) * 0.05, "ba": torch.randn(A, generator=g)}
    Pon, Ptg = P(), P()
    act = torch.randint(0, A, (B,), generator=g).to(torch.int32)
    rew = torch.randn(B, generator=g) * 3
    gam = torch.full((B,), 0.97)
    gam[::7] = 0.0
    isw = torch.rand(B, generator=g)

    def E():
        return {"wtau": torch.randn(1024, 64, generator=g) * 0.125, "btau": torch.randn(1024, generator=g) * 0.1 ** 0.5}
    Eon, Etg = E(), E()
    if split:
        (Hon, Hon_lo), (Htg, Htg_lo) = split_planes(Hon), split_planes(Htg)
    else:
        Hon, Htg, Hon_lo, Htg_lo = Hon.to(torch.bfloat16), Htg.to(torch.bfloat16), None, None
    return dict(Hon=Hon, Htg=Htg, Hon_lo=Hon_lo, Htg_lo=Htg_lo, Pon=Pon, Ptg=Ptg, Eon=Eon, Etg=Etg, act=act, rew=rew,
                gam=gam, isw=isw)


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
        assert case in ("plain", "kappa"), case
    return rew, gam, isw


GRADS = ("wv", "bv", "wa", "ba", "wtau", "btau")


def run_torch(B, A, N, split=False, case="plain", kappa=KAPPA, dtype=torch.float64):
    """The torch backend in ``dtype`` on the joined activations of ``fixture(B, A, split)``: every output
    of the head and of the weight gradient, plus the oracle's own diagnostics."""
    from apex_dqn_amd.ops.fused_ops import TorchBackend
    be = TorchBackend(dtype)
    fx = fixture(B, A, split)
    rew, gam, isw = case_inputs(fx, case)
    d = lambda t: t.to(dtype)                                            # noqa: E731
    join = lambda hi, lo: d(hi) if lo is None else d(hi.double() + lo.double())     # noqa: E731
    Hon, Htg = join(fx["Hon"], fx["Hon_lo"]), join(fx["Htg"], fx["Htg_lo"])
    Pon, Ptg = {k: d(v) for k, v in fx["Pon"].items()}, {k: d(v) for k, v in fx["Ptg"].items()}
    Eon, Etg = {k: d(v) for k, v in fx["Eon"].items()}, {k: d(v) for k, v in fx["Etg"].items()}
    z = lambda *s: torch.zeros(*s, dtype=dtype)                          # noqa: E731
    td, loss, dH, dhead, q = z(B), z(B), z(B, 1024), z(B, (A + 1) * N), z(B, A)
    taus = torch.zeros(B, 3, N)
    ws = be.iqn_workspace(B, N, "cpu", dtype)
    ctr, base = torch.tensor([CTR]), torch.tensor([BASE])
    stat = (torch.full((1,), WSCALE), torch.full((1,), -1.0, dtype=torch.float64), torch.zeros((), dtype=torch.int64))
    be.iqn_head(Hon, Htg, Pon, Ptg, Eon, Etg, fx["act"], d(rew), d(gam), None if isw is None else d(isw), N, kappa,
                1.0 / B, seed_q(), ctr, base, td, loss, dH, dhead, ws, q_out=q, tau_out=taus,
                isn=None if isw is None else stat)
    gr = {"wv": z(1, 512), "bv": z(1), "wa": z(A, 512), "ba": z(A), "wtau": z(1024, 64), "btau": z(1024)}
    be.iqn_wgrad(fx["act"], ws, gr)
    out = dict(td=td, loss=loss, dH=dH, dhead=dhead, q=q, g=gr, taus=taus, isn=float(stat[1]), count=int(stat[2]))
    if dtype == torch.float64:
        # diagnostics of the oracle alone: the top-2 gap of the online next-state q, the taken action's
        # quantiles and target samples, and the near-kink slack of the embedding's gradient rows
        th_n, _, _ = be._iqn_theta(Hon[B:2 * B], Pon, Eon, taus[:, 1], dtype)
        qn = th_n.mean(-1)
        top = qn.topk(2, dim=1).values
        ar = torch.arange(B)
        th_t, pre, _ = be._iqn_theta(Hon[:B], Pon, Eon, taus[:, 0], dtype)
        th_g = be._iqn_theta(Htg[:B], Ptg, Etg, taus[:, 2], dtype)[0][ar, qn.argmax(1)]
        near = pre.abs() < KINK                                          # [B, N, 1024]
        g = dhead[:, :N]
        coef = torch.nn.functional.one_hot(fx["act"].long(), A).double() - 1.0 / A
        dxv = g[:, :, None] * Pon["wv"].reshape(512)
        dxa = g[:, :, None] * (coef @ Pon["wa"])[:, None, :]
        unmasked = (torch.cat([dxv, dxa], -1) * Hon[:B, None, :]).abs()
        out.update(gap=float((top[:, 0] - top[:, 1]).min()), th=th_t[ar, fx["act"].long()], th_target=th_g,
                   slack=(unmasked * near).sum((0, 1)), kink_share=float(near.any(0).any(0).float().mean()))
    return out


@functools.lru_cache(maxsize=None)
def oracle(B, A, N, split=False, case="plain", kappa=KAPPA):
    """fp64 CPU oracle (computed once per problem, shared, never modified)."""
    return run_torch(B, A, N, split, case, kappa, torch.float64)


def compare(h, r):
    """The tolerances of ``_compare`` in tests/test_gpu_qr.py, and for the embedding's gradients the head
    gradients' tolerance plus the near-kink slack of the row (``r["slack"]``)."""
    f = lambda t: t.float()                                              # noqa: E731
    torch.testing.assert_close(f(h["td"]), f(r["td"]), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(f(h["loss"]), f(r["loss"]), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(f(h["dH"]), f(r["dH"]), rtol=1e-2, atol=1e-6)
    torch.testing.assert_close(f(h["dhead"]), f(r["dhead"]), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(f(h["q"]), f(r["q"]), rtol=1e-4, atol=1e-4)
    for k in ("wv", "bv", "wa", "ba"):
        torch.testing.assert_close(f(h["g"][k]), f(r["g"][k]), rtol=1e-3, atol=1e-6)
    slack = r["slack"]
    for k, s in (("wtau", slack[:, None]), ("btau", slack)):
        ref = r["g"][k]
        err = (h["g"][k].double() - ref).abs()
        bound = 1e-6 + 1e-3 * ref.abs() + s
        assert bool((err <= bound).all()), (k, float((err - bound).max()))


def max_errors(h, r):
    """Largest error of every output in units of its tolerance (<= 1 passes), for the reports."""
    tol = dict(td=(1e-4, 1e-4), loss=(1e-4, 1e-5), dH=(1e-2, 1e-6), dhead=(1e-4, 1e-7), q=(1e-4, 1e-4))
    out = {}
    for k, (rt, at) in tol.items():
        out[k] = float(((h[k].double() - r[k]).abs() / (at + rt * r[k].abs())).max())
    for k in GRADS:
        s = 0.0 if k not in ("wtau", "btau") else (r["slack"][:, None] if k == "wtau" else r["slack"])
        ref = r["g"][k]
        out["g_" + k] = float(((h["g"][k].double().reshape(ref.shape) - ref).abs() / (1e-6 + 1e-3 * ref.abs() + s)).max())
    return out
