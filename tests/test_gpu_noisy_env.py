"""Per-environment actor noise on the GPU (csrc/noisy_actor.hip): the draw against the host mirror and the shared
draw, the dual-operand fc GEMM and the logits / finish launches against the fp64 oracles on a given Xi, and the actor
group against the torch backend, under graph replay and on identical frames."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 1e-4          # tests/test_gpu_split.py TOL: relative L2 of the split-mode kernels vs fp64
ROW_TILE = 64       # rows of a noisy_env_fc_kernel / noisy_env_logits_kernel block


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _flat(A, N):
    """Flat parameters (device) in the noisy layout: mu ~ U(-0.05, 0.05), sigma ~ U(0, 0.02), as tests/test_gpu_noisy.py."""
    from apex_dqn_amd.models.flat_params import FlatLayout, nature_segments
    lay = FlatLayout(nature_segments(4, A, 64, N, noisy=True))
    g = torch.Generator().manual_seed(11)
    p = (torch.rand(lay.numel, generator=g) - 0.5) * 0.1
    for s in ("swv", "sbv", "swa", "sba", "swfc", "sbfc"):
        o, n = lay.offsets[s], int(np.prod(lay.shapes[s]))
        p[o:o + n] = torch.rand(n, generator=g) * 0.02
    return lay, FlatLayout(nature_segments(4, A, 64, N)), p.to(DEV)


def _plan(A, N, ctr, s=5, every=1):
    from apex_dqn_amd.learner.noisy import NoisyPlan, noise_seed
    return NoisyPlan(A=A, N=N, offsets=dict(_flat(A, N)[0].offsets), seed=noise_seed(3),
                     ctr=torch.tensor([ctr], dtype=torch.int64, device=DEV), every=every, stream0=s)


def _given_xi(E, K, seed, same_rows=False):
    """A random Xi [E, K padded to 64] of the draws' scale (xi = sign(g) sqrt|g|)."""
    g = torch.randn(1 if same_rows else E, K, generator=torch.Generator().manual_seed(seed))
    xi = torch.zeros(E, (K + 63) // 64 * 64)
    xi[:, :K] = torch.sign(g) * g.abs().sqrt()
    return xi.to(DEV)


@pytest.mark.parametrize("A,N", [(4, 1), (3, 7)])
@pytest.mark.parametrize("E", [1, 5])
def test_env_draw_vs_mirror_shared_draw_and_graph(E, A, N):
    """Every row against the fp64 mirror at tests/test_gpu_noisy.py's bound on the Gaussians (2e-5, derived there); row 0
    bit-equal to the xi noisy_compose writes for the same (u, s); a graph replayed twice draws for ctr and ctr + 1."""
    from apex_dqn_amd.learner.noisy import gaussians
    from apex_dqn_amd.ops.fused_ops import HipBackend
    be, u = HipBackend(), 123457
    plan = _plan(A, N, u)
    K = plan.K
    xi = torch.full((E, (K + 63) // 64 * 64), -9.0, device=DEV)
    be.noisy_env_draw(plan, xi)
    torch.cuda.synchronize()
    assert bool((xi[:, K:] == -9.0).all())
    for e in range(E):
        x = xi[e, :K].cpu().double()
        err = float((torch.sign(x) * x * x - torch.from_numpy(gaussians(plan.seed, u, 5, K, e))).abs().max())
        assert err <= 2e-5, (e, err)
    lay, mu, p = _flat(A, N)
    shared = torch.zeros(1, xi.shape[1], device=DEV)
    be.noisy_compose(plan, [(p, torch.zeros(mu.numel, device=DEV),
                             torch.zeros(mu.numel, device=DEV, dtype=torch.bfloat16), None)], shared)
    torch.cuda.synchronize()
    assert torch.equal(xi[0, :K], shared[0, :K])
    want = []
    for c in (u + 1, u + 2):
        w = torch.zeros_like(xi)
        be.noisy_env_draw(_plan(A, N, c), w)
        want.append(w)
    plan.ctr.fill_(u + 1)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        be.noisy_env_draw(plan, xi)         # warm
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            be.noisy_env_draw(plan, xi)
            plan.ctr += 1
        for w in want:
            g.replay()
            st.synchronize()
            assert torch.equal(xi[:, :K], w[:, :K])
    assert not torch.equal(want[0], want[1])


def _fc_inputs(E, split):
    lay, _, p = _flat(4, 1)
    plan = _plan(4, 1, 0)
    x32 = torch.relu(torch.randn(E, 3136, generator=torch.Generator().manual_seed(E))).to(DEV)
    planes = lambda t: (t.to(torch.bfloat16), (t - t.to(torch.bfloat16).float()).to(torch.bfloat16) if split else None)  # noqa: E731
    seg = {k: plan.seg(p, k).contiguous() for k in ("wfc", "swfc", "bfc", "sbfc")}
    return plan, p, seg, planes(x32), planes(seg["wfc"]), planes(seg["swfc"])


def _run_fc(E, split, xi):
    from apex_dqn_amd.ops.fused_ops import HipBackend
    plan, p, seg, (x, xl), (w, wl), (sw, swl) = _fc_inputs(E, split)
    buf = [torch.full((E * 1024 + 256,), 3.0, device=DEV, dtype=torch.bfloat16) for _ in range(2)]
    h, hl = buf[0][:E * 1024].view(E, 1024), buf[1][:E * 1024].view(E, 1024) if split else None
    HipBackend().noisy_env_fc(x, w, sw, seg["bfc"], seg["sbfc"], xi, h, x_lo=xl, w_lo=wl, sw_lo=swl, out_lo=hl)
    torch.cuda.synchronize()
    assert bool((buf[0][E * 1024:] == 3.0).all()) and bool((buf[1][E * 1024:] == 3.0).all())      # the canaries
    return h, hl


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("E", [1, 5, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1])
def test_env_fc_vs_fp64(E, split):
    """h against the fp64 formula on the fp32 mu / sigma, the activation planes as given and a given Xi.  fp32-class:
    tests/test_gpu_split.py's bound on the fc forward.  bf16: all rows of Xi equal one draw, the parent path
    (noisy_compose + fc_fwd on the same inputs) is measured against the same reference, and the kernel may err twice
    that (one extra bf16 rounding, of the gated operand).  Two launches are bit-identical; nothing behind h is written."""
    from apex_dqn_amd.ops.fused_ops import HipBackend, TorchBackend, join
    plan, p, seg, (x, xl), _, _ = _fc_inputs(E, split)
    xi = _given_xi(E, plan.K, 7 + E, same_rows=not split)
    h, hl = _run_fc(E, split, xi)
    ref = torch.zeros(E, 1024, dtype=torch.float64, device=DEV)
    TorchBackend().noisy_env_fc(join(x, xl, torch.float64), seg["wfc"].double(), seg["swfc"].double(), seg["bfc"].double(),
                                seg["sbfc"].double(), xi.double(), ref)
    err = _rel(join(h, hl, torch.float64), ref)
    if split:
        bound = TOL
    else:
        _, mu, _ = _flat(4, 1)
        e32 = torch.zeros(mu.numel, device=DEV)
        ebf = torch.zeros(mu.numel, device=DEV, dtype=torch.bfloat16)
        TorchBackend().noisy_compose(plan, [(p, e32, ebf, None)], torch.zeros_like(xi[:1]), xi_in=xi[:1])
        hp = torch.zeros(E, 1024, device=DEV, dtype=torch.bfloat16)
        HipBackend().fc_fwd(x, plan.seg(ebf, "wfc"), plan.seg(e32, "bfc"), hp)
        torch.cuda.synchronize()
        bound = 2.0 * _rel(hp, ref)
    print(f"E = {E} split {split}: relative L2 error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)
    h2, hl2 = _run_fc(E, split, xi)
    assert torch.equal(h.view(torch.int16), h2.view(torch.int16))
    assert not split or torch.equal(hl.view(torch.int16), hl2.view(torch.int16))


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("E", [5, ROW_TILE + 1])
@pytest.mark.parametrize("A,N,kind", [(4, 1, "scalar"), (18, 1, "scalar"), (3, 7, "quantile"), (4, 51, "categorical"),
                                      (4, 101, "categorical")])
def test_env_logits_and_finish_vs_fp64(A, N, kind, E, split):
    """q against the fp64 oracle on the kernel's own h and a given Xi at the existing actor-head tests' tolerances
    (scalar: rtol = atol = 1e-4, tests/test_gpu_ddqn_head.py; quantile / categorical: 1e-4 absolute,
    tests/test_gpu_qr_wide.py, tests/test_gpu_cat_wide.py); with eps = 0.9 the actions are the host mirror of the draw
    (words 2 e, 2 e + 1 of the counter RNG) applied to the kernel's own q."""
    from apex_dqn_amd.ops.fused_ops import HipBackend, TorchBackend, join
    from apex_dqn_amd.replay.gpu_replay import apex_uniform
    _, _, p = _flat(A, N)
    plan = _plan(A, N, 0)
    xi = _given_xi(E, plan.K, 31 * A + N)
    h, hl = _run_fc(E, split, xi)
    P = {k: plan.seg(p, k).contiguous() for k in ("wv", "bv", "wa", "ba")}
    S = {k: plan.seg(p, "s" + k).contiguous() for k in ("wv", "bv", "wa", "ba")}
    head = {"scalar": ("scalar",), "quantile": ("quantile", N), "categorical": ("categorical", N, -10.0, 10.0)}[kind]
    eps, ctr = torch.full((E,), 0.9, device=DEV), torch.full((1,), 3, dtype=torch.int64, device=DEV)
    tb, be = TorchBackend(), HipBackend()
    d = lambda D: {k: v.double() for k, v in D.items()}      # noqa: E731
    L64 = tb.noisy_env_logits_ws(E, A, N, DEV, dtype=torch.float64)
    q_ref, a_ref = torch.zeros(E, A, dtype=torch.float64, device=DEV), torch.zeros(E, dtype=torch.int32, device=DEV)
    tb.noisy_env_logits(join(h, hl, torch.float64), d(P), d(S), xi.double(), N, L64)
    tb.noisy_env_finish(h, L64, d(P), eps, ctr, 5, head, q_ref, a_ref)
    L = be.noisy_env_logits_ws(E, A, N, DEV)
    q, a = torch.full((E, A), 11.0, device=DEV), torch.full((E,), -3, dtype=torch.int32, device=DEV)
    be.noisy_env_logits(h, P, S, xi, N, L, H_lo=hl)
    be.noisy_env_finish(h, L, P, eps, ctr, 5, head, q, a)
    torch.cuda.synchronize()
    err = float((q.double() - q_ref).abs().max())
    print(f"(A, N) = ({A}, {N}) {kind} E = {E} split {split}: max |q - q_ref| = {err:.2e} (|q| max {float(q_ref.abs().max()):.2e})")
    if kind == "scalar":
        torch.testing.assert_close(q, q_ref.float(), rtol=1e-4, atol=1e-4)
    else:
        assert err < 1e-4, err
    e = np.arange(E)
    u, rr = apex_uniform(5, 3, 2 * e), apex_uniform(5, 3, 2 * e + 1)
    want = np.where(u < np.float32(0.9), np.minimum((rr * np.float32(A)).astype(np.int64), A - 1), q.cpu().numpy().argmax(1))
    assert np.array_equal(a.cpu().numpy(), want) and 0 < int((u < np.float32(0.9)).sum()) < E


def _group(backend, E, frames_seed=5, **rt):
    from apex_dqn_amd.actors.gpu_actor import GpuActorGroup
    from apex_dqn_amd.config import ApexConfig
    from apex_dqn_amd.envs.vector_envs import make_vec_env
    from apex_dqn_amd.learner.fused_learner import FusedNatureLearner
    from apex_dqn_amd.replay.gpu_replay import GpuReplayShard
    A = 6
    rt.setdefault("actor_graph", backend == "hip")      # (the torch backend reads the draw index back: no capture)
    cfg = ApexConfig.from_dict({"env_conf": {"state_shape": [4, 84, 84], "action_dim": A, "name": "Synthetic"},
                                "Actor": {"num_actors": E, "epsilon": 0.0}, "Learner": {"replay_sample_size": 32},
                                "Runtime": {"use_graphs": False, "dtype": "fp32", "noisy": True, "seed": 4,
                                            "noisy_actor_noise": "per_env", **rt}})
    torch.manual_seed(3)
    rp = GpuReplayShard(1000, 1000, 1200, 4, device=DEV)
    L = FusedNatureLearner(cfg, DEV, rp, backend=backend, split=True)
    with torch.no_grad():
        for s in ("swv", "sbv", "swa", "sba", "swfc", "sbfc"):
            L.P[s].mul_(4.0)                       # a visible noise term
    L._refresh_bf16()
    grp = GpuActorGroup(cfg, L, rp, make_vec_env(cfg.env_backend, cfg.env_conf.name, E, A, seed=0), E, group=1)
    assert grp.env_noise and grp.split and grp.xi.shape[0] == E
    seqs = rp.append_frames(np.random.default_rng(frames_seed).integers(0, 255, (E + 8, 84, 84), dtype=np.uint8))
    return grp, seqs


@pytest.mark.parametrize("num_atoms,kind", [(1, "categorical"), (7, "quantile")])
def test_env_noise_group_hip_vs_torch_backend(num_atoms, kind):
    """One call of the group on the HIP backend against the same group on the torch backend at the bound of
    tests/test_gpu_noisy.py's actor-group test (1e-4 absolute, split kernels); identical frames in every env give
    differing q rows."""
    E, qs = 24, {}
    for be in ("hip", "torch"):
        grp, seqs = _group(be, E, num_atoms=num_atoms, dist_head=kind)
        qs[be], a = grp.policy(np.stack([seqs[i:i + 4] for i in range(E)]))
        assert np.array_equal(a, qs[be].argmax(1)) and int(grp.ctr) == 1
    err = float(np.abs(qs["hip"] - qs["torch"]).max())
    print(f"N = {num_atoms} {kind}: max |q_hip - q_torch| = {err:.2e} (|q| max {float(np.abs(qs['torch']).max()):.2e})")
    assert err < 1e-4, err
    q, _ = grp.policy(np.repeat(seqs[None, :4], E, axis=0))
    assert min(float(np.abs(q[i] - q[j]).max()) for i in range(3) for j in range(i + 1, 4)) > 1e-3


def test_env_noise_group_graph_replays_equal_eager_calls():
    """Three replays of the captured actor call are bit-equal to three eager calls, under three different draws."""
    E, res = 24, {}
    for graph in (True, False):
        grp, seqs = _group("hip", E, actor_graph=graph, num_atoms=51)
        payload = np.stack([seqs[i:i + 4] for i in range(E)])
        out = []
        for call in range(3):
            assert int(grp.ctr) == call
            q, a = grp.policy(payload)
            out.append((q, a, grp.xi.clone()))
        assert (getattr(grp, "_graph", None) is not None) == graph
        res[graph] = out
    for (q0, a0, x0), (q1, a1, x1) in zip(res[True], res[False]):
        assert np.array_equal(q0, q1) and np.array_equal(a0, a1) and torch.equal(x0, x1)
    assert not torch.equal(res[True][0][2], res[True][1][2]) and not torch.equal(res[True][1][2], res[True][2][2])
    assert float(np.abs(res[True][0][0] - res[True][1][0]).max()) > 1e-3
