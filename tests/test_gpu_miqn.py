"""Munchausen-IQN (``Runtime.dist_head = "implicit_munchausen"``) on the GPU: the three launches of csrc/iqn_wide_head.hip
``apex_miqn_wide_head`` and the weight gradient against the fp64 oracle, at the bounds tests/test_miqn_cpu.py measures;
the launcher's refusals, captured replays, the whole step against the torch backend and graph replay."""
import iqn_fixtures as F
import pytest
import torch
from test_gpu_iqn import DEV, _cfg, _dev, _fill_replay
from test_miqn_cpu import CASES, EDGE, MK, SHAPES, allowances, compare, fixture, oracle

pytestmark = pytest.mark.gpu
GRADS = {"wv": (1, 512), "bv": (1,), "wa": (None, 512), "ba": (None,), "wtau": (1024, 64), "btau": (1024,)}


def _run_hip(B, A, N, split=False, case="plain", max_blocks=None, graph=0, **bad):
    """The head and the weight gradient on ``fixture``; ``graph``: captured once, replayed that many times; ``bad``:
    arguments overridden for the launcher's refusals (then the status is returned with the outputs)."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be, fx, mk = HipBackend(), fixture(B, A, split), {**MK, **CASES.get(case, {}), **bad}
    rew, gam, isw = F.case_inputs(fx, "plain" if case in CASES else case)
    P = {n: {k: _dev(v) for k, v in fx[n].items()} for n in ("Pon", "Ptg", "Eon", "Etg")}
    td, loss = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    dH = torch.zeros(B, 1024, device=DEV, dtype=torch.bfloat16)
    dH_lo = torch.zeros_like(dH) if split else None
    dhead, q, aux = torch.full((B, (A + 1) * N), 7.0, device=DEV), torch.zeros(B, A, device=DEV), torch.zeros(B, 2, device=DEV)
    taus, ws = torch.full((B, 3, N), -1.0, device=DEV), be.iqn_workspace(B, N, DEV)
    gr = {k: torch.zeros([A if d is None else d for d in s], device=DEV) for k, s in GRADS.items()}
    flat, L = torch.full((64,), 3.0, device=DEV), be.qr_wide_logits(3 * B, A, N, DEV)
    args = [_dev(t) for t in (fx["Hon"], fx["Htg"])] + [P["Pon"], P["Ptg"], P["Eon"], P["Etg"]] + [
        _dev(t) for t in (fx["act"], rew, gam, isw)]
    ctr, base = torch.tensor([F.CTR], device=DEV), torch.tensor([F.BASE], device=DEV)

    def run():
        be.miqn_head(*args, N, F.KAPPA, mk["alpha"], mk["tau"], mk["clip"], 1.0 / B, F.seed_q(), ctr, base, td, loss, dH,
                     dhead, ws, aux=None if "aux" in bad else aux, q_out=q, tau_out=taus, zero=flat,
                     lo=(_dev(fx["Hon_lo"]), _dev(fx["Htg_lo"]), dH_lo) if split else None, max_blocks=max_blocks, logits=L,
                     rescale_eps=bad.get("rescale_eps"))
        be.iqn_wgrad(args[6], ws, gr)
    if bad:
        with pytest.raises(RuntimeError, match="miqn_wide_head"):
            run()
    elif graph:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            run()                                        # (the launcher raises its LDS bound outside the capture)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                run()
        for _ in range(graph):
            g.replay()
    else:
        run()
    torch.cuda.synchronize()
    dHj = dH.double() + (dH_lo.double() if split else 0.0)
    return dict(td=td.cpu(), loss=loss.cpu(), dH=dHj.cpu(), dhead=dhead.cpu(), q=q.cpu(), taus=taus.cpu(),
                bonus=aux[:, 0].cpu(), vsoft=aux[:, 1].cpu(), g={k: v.cpu() for k, v in gr.items()},
                zeroed=bool((flat == 0).all()), dpre=ws["dpre"].cpu())


def _same_bits(a, b):
    for k in ("td", "loss", "dH", "dhead", "q", "taus", "bonus", "vsoft", "dpre"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(a["g"][k], b["g"][k]) for k in GRADS)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,A,N", SHAPES)
def test_miqn_head_and_wgrad_vs_fp64_oracle(B, A, N, split):
    """Every output within the wide implicit head's bounds plus tests/test_miqn_cpu.py's measured allowances; the
    fractions equal the mirror's bit for bit (set 1 on the S_t target rows); one block that walks all 3B rows across
    the net switch at row B leaves the default grid's bits."""
    r, h = oracle(B, A, N, split), _run_hip(B, A, N, split)
    assert torch.equal(h["taus"], r["taus"]) and h["zeroed"]
    compare(h, r, *allowances(B, A, N, split))
    if A == 1:
        assert not bool(h["bonus"].any())
    _same_bits(h, _run_hip(B, A, N, split, max_blocks=1))


@pytest.mark.parametrize("case", ["terminal", "no_isw", "alpha0", "tau1"])
def test_miqn_edge_cases(case):
    r, h = oracle(*EDGE, False, case), _run_hip(*EDGE, False, case)
    compare(h, r, *allowances(*EDGE, False, case))
    if case == "alpha0":
        assert not bool(h["bonus"].any())


@pytest.mark.parametrize("bad", [dict(tau=0.0), dict(alpha=1.5), dict(clip=0.0), dict(aux=None), dict(rescale_eps=1e-2)])
def test_miqn_launcher_refuses(bad):
    """hipErrorInvalidValue and nothing launched: the outputs keep their fill."""
    h = _run_hip(4, 2, 65, **bad)
    assert bool((h["td"] == -1).all()) and bool((h["dhead"] == 7).all()) and not h["zeroed"] and not bool(h["dpre"].any())


def test_miqn_captured_launches_replay_to_the_eager_bits():
    _same_bits(_run_hip(*EDGE, graph=4), _run_hip(*EDGE))


def _learner(cfg, backend="hip", split=False, seed=7, fill=11):
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    torch.manual_seed(0)
    rp = GpuReplayShard(2000, 2000, 2100, 4, device=DEV, seed=seed)
    _fill_replay(rp, 1500, seed=fill)
    return FusedNatureLearner(cfg, DEV, rp, backend=backend, split=split), rp


MIQN = dict(num_atoms=72, dist_head="implicit_munchausen", iqn_wide=True)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_miqn_learner_step_hip_vs_torch_backend(dtype):
    """tests/test_gpu_iqn_wide.py's whole-step test and bounds on the Munchausen row plan, with the two metrics."""
    split, res = dtype == "fp32", {}
    cfg = _cfg(32, use_graphs=False, presample=False, dtype=dtype, **MIQN)
    for be in ("hip", "torch"):
        L, _ = _learner(cfg, be, split)
        assert L.miqn and L.m_plan and L._rows_first == 32 and L.split == split
        if be == "torch":
            L.ops.dtype = torch.float32
        L._step_body()
        torch.cuda.synchronize()
        m = L.last_metrics()
        res[be] = (L.td_abs.clone(), L.loss_b.clone(), L.layout.views(L.g32.clone()), L.tau_out.clone(),
                   torch.tensor([m["munchausen_bonus_mean"], m["soft_value_mean"]]))
    assert torch.equal(res["hip"][3], res["torch"][3])
    for i in (0, 1, 4):
        torch.testing.assert_close(res["hip"][i], res["torch"][i], rtol=5e-2, atol=5e-2)
    gh, gt = res["hip"][2], res["torch"][2]
    errs = {k: float((gh[k] - gt[k]).norm() / (gt[k].norm() + 1e-12)) for k in gh}
    print(f"per-segment relative grad error ({dtype}):", errs)
    assert max(errs.values()) < 0.2 and float(gt["wtau"].norm()) > 0, errs


def test_miqn_graph_replay_is_bit_identical_to_eager():
    res = {}
    for graphs in (True, False):
        L, rp = _learner(_cfg(32, use_graphs=graphs, graph_steps=4, learner={"q_target_sync_freq": 1000}, **MIQN),
                         seed=3, fill=1)
        L.steps(4) if graphs else [L.step() for _ in range(4)]
        torch.cuda.synchronize()
        assert L.num_q_updates == 4 and (L._multi is not None) == graphs
        res[graphs] = (L.p32.clone(), L.t32.clone(), rp.leaf.clone(), L.td_abs.clone(), L.mdqn_aux.clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
