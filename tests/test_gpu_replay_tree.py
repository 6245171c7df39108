"""The prioritized-replay kernels (csrc/sumtree.hip) against the host model of
tests/test_replay_tree_cpu.py, at the tree sizes where the code changes path: ``L == 1``, a last
parent with a single child, the LDS accumulator of ``tree_block_update`` exactly full
(258 048 leaves, ``kfirst == 1``) and the two-tier update (``kfirst == 2`` from 258 049 leaves:
level 1 takes one fp64 global atomic per leaf, the levels above are summed in LDS first).

Every level of the tree is compared, not only the root: a delta added to the wrong level-1 or
level-2 node leaves the root exact and silently skews which leaves are sampled.

Running minimum: the kernels fold every positive value they write into one atomicMin word, so
between two ``rebuild()`` calls ``min_leaf()`` is a lower bound of the true minimum over the
live leaves -- equal to it until the minimum leaf is overwritten with a larger value or evicted,
``0 < min_leaf() <= true_min()`` afterwards; ``rebuild()`` restores equality.  (The CPU path
recomputes it on every mutation and is exact: test_replay_tree_cpu.py.)"""
import math

import numpy as np
import pytest
import torch

from test_replay_tree_cpu import (Driver, TreeModel, check_exact_draw, check_records, check_sample, kfirst,
                                  random_ops, tree_sizes)

from apex_dqn_amd.replay.gpu_replay import GpuReplayShard, apex_uniform

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(64, 1), (4097, 1), (258_048, 1), (258_049, 2), (391_649, 2)]     # (capacity, kfirst)
BIG = 258_049                                                               # the smallest two-tier tree


def _shard(cap, seed=5, **kw):
    return GpuReplayShard(cap, cap, 64, 4, device=DEV, seed=seed, **kw)


def _pair(cap, seed=5, **kw):
    rp = _shard(cap, seed, **kw)
    return rp, TreeModel(cap, 4, rp.alpha, rp.eps)


def _filled(cap, seed=1, **kw):
    """A shard whose slots [0, cap - min(cap // 4, 1500)) are live (the op sequence's first insert)."""
    rp, m = _pair(cap, **kw)
    drv = Driver(rp, m)
    drv.apply(next(random_ops(np.random.default_rng(seed), cap, 1)))
    return rp, m, drv


def _clone(rp):
    q = _shard(rp.cap, rp.seed, alpha=rp.alpha, eps=rp.eps, beta=rp.beta)
    for name in ("leaf", "nodes", "min_bits", "obs", "nxt", "act", "rew", "gam", "gen", "ctr"):
        getattr(q, name).copy_(getattr(rp, name))
    q.head, q.live = rp.head, rp.live
    return q


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_tree(rp, m, worst=None):
    """Leaves vs the model (rtol 2e-6, same live set); every node of every level vs the exact sums
    of the leaves read back from the device, within the model's round-off bound; the minimum.
    ``worst[k]`` collects the largest error / bound ratio per level.  Returns the device leaves."""
    torch.cuda.synchronize()
    leaf = rp.leaf.cpu().numpy()
    nodes = rp.nodes.cpu().numpy()
    np.testing.assert_allclose(leaf, m.leaf, rtol=2e-6)
    np.testing.assert_array_equal(leaf > 0, m.leaf > 0)
    for k, exact in enumerate(m.levels(leaf)):
        if k == 0:
            continue
        got = nodes[rp.offs[k]:rp.offs[k] + rp.sizes[k]]
        err, bound = np.abs(got - exact), m.node_bound(k)
        ratio = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)))
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), ratio)
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, (f"level {k} of {rp.L}: {bad.size} nodes off, first {bad[:5]}, "
                               f"err {err[bad[:5]]}, bound {bound[bad[:5]]}, touch {m.touch[k][bad[:5]]}")
    mn, tm = rp.min_leaf(), m.true_min(leaf)
    assert 0 < mn <= tm, (mn, tm)
    if not m.min_stale:
        assert mn == tm, (mn, tm)
    return leaf


# ------------------------------------------------------------ 1. op sequence
@pytest.mark.parametrize("cap,kf", SHAPES)
def test_op_sequence_matches_model_at_every_level(cap, kf):
    """~30 inserts (some wrapping the ring over live leaves), updates, evictions, samples and
    rebuilds; after every op: leaves at rtol 2e-6, records and generations bit-equal, every node
    within ``touch * 2**-52 * peak`` of the exact sum of the device's own leaves (plus the
    summation-order term an exact rebuild leaves, 64 * 2**-53 relative per level -- all that is
    allowed right after ``rebuild()``), and the running minimum a lower bound that is exact
    until the minimum leaf was raised or removed (module docstring)."""
    assert kfirst(tree_sizes(cap)) == kf
    rp, m = _pair(cap)
    assert rp.sizes == tree_sizes(cap) and rp.L == len(rp.sizes) - 1
    drv = Driver(rp, m)
    worst, kinds, wrapped, stale_seen = {}, set(), False, False
    for op in random_ops(np.random.default_rng(cap), cap, 30):
        h0 = drv.head
        drv.apply(op)
        kinds.add(op[0])
        wrapped |= op[0] == "insert" and drv.head <= h0
        leaf = check_tree(rp, m, worst)
        check_records(rp, m)
        stale_seen |= m.min_stale
        if op[0] == "sample":
            B, out = drv.last_sample
            check_sample(rp, m, B, out, leaf, int(rp.ctr.item()))
    print(f"cap {cap} L {rp.L} kfirst {kf} max node error / bound per level {worst} "
          f"max touches {[int(t.max()) for t in m.touch[1:]]}")
    rp.rebuild()
    m.rebuilt()
    check_tree(rp, m)
    assert {"insert", "update", "evict", "sample"} <= kinds and wrapped and m.gen.max() >= 2


# ------------------------------------------------------- 2. dynamic range
def test_large_dynamic_range_drift_and_rebuild():
    """2 000 leaves of the two-tier tree raised to ~1e4 and then dropped to ~1e-4 (leaves of
    ~1 around them): the nodes keep the absolute round-off of their peak, which the per-node
    bound allows and nothing more; rebuild() restores the exact sums."""
    rp, m, drv = _filled(BIG, eps=1e-9)
    rng = np.random.default_rng(2)
    sel = rng.choice(BIG - 1500, 2000, replace=False).astype(np.int64)
    sel[:64] = 64 * 70 + np.arange(64)            # one level-1 node moves as a whole
    worst = {}
    for target in (1e4, 1e-4):
        td = (target ** (1.0 / rp.alpha) * (0.5 + rng.random(2000))).astype(np.float32)
        for a in range(0, 2000, 1000):
            rp.update_priorities(_dev(sel[a:a + 1000]), _dev(td[a:a + 1000]), _dev(m.gen[sel[a:a + 1000]]))
            m.update(sel[a:a + 1000], td[a:a + 1000], m.gen[sel[a:a + 1000]])
            leaf = check_tree(rp, m, worst)
        assert 0.3 * target < np.median(leaf[sel]) < 3 * target
    print(f"dynamic range: max node error / bound per level {worst}")
    rp.rebuild()
    m.rebuilt()
    check_tree(rp, m)


# ------------------------------------------------------------ 3. exact draw
_STATES = {}


def _drawn_state(cap):
    """A tree after 12 ops (wrapped inserts, evicted ranges, updated leaves), shared read-only."""
    if cap not in _STATES:
        rp, m = _pair(cap)
        drv = Driver(rp, m)
        for op in random_ops(np.random.default_rng(100 + cap), cap, 12):
            if op[0] != "sample":
                drv.apply(op)
        _STATES[cap] = (rp, m, check_tree(rp, m))
    return _STATES[cap]


@pytest.mark.parametrize("B", [1, 3, 64, 512, 1000])
@pytest.mark.parametrize("cap,kf", SHAPES)
def test_sample_lands_on_the_reconstructed_draw(cap, kf, B):
    """u_b = (b + U(seed, ctr, b)) * root / B recomputed on the host: the sampled leaf is live and
    its mass interval holds u_b (1e-9 of the total as margin), for every row; IS weights with the
    kernel's running minimum; gathered records bit-equal."""
    rp, m, leaf = _drawn_state(cap)
    seed0 = rp.seed
    try:
        for seed in (seed0, 0x9E3779B97F4A7C15):
            for ctr in (0, 1, 2 ** 40 + 3):
                rp.seed = seed
                rp.ctr.fill_(ctr)
                out = rp.sample(B)
                torch.cuda.synchronize()
                check_sample(rp, m, B, out, leaf, ctr)
    finally:
        rp.seed = seed0


# ----------------------------------------------------------------- 4. holes
def _full(cap):
    rp, m = _pair(cap)
    drv = Driver(rp, m)
    rng = np.random.default_rng(cap + 7)
    gen = random_ops(rng, cap, 3)
    first = next(gen)
    drv.apply(first)
    rest = cap - len(first[2])
    drv.apply(("insert", {k: v[:rest] for k, v in first[1].items()}, first[2][:rest]))     # ring full, head 0
    assert drv.head == 0 and drv.live == cap
    return rp, m, drv, first


def _layout(cap, name):
    if name == "leaf0":
        rp, m = _pair(cap)
        drv = Driver(rp, m)
        first = next(random_ops(np.random.default_rng(3), cap, 1))
        drv.apply(("insert", {k: v[:1] for k, v in first[1].items()}, first[2][:1]))
        return rp, m
    rp, m, drv, first = _full(cap)
    if name == "last_leaf":
        drv.apply(("evict", cap - 1))
        assert np.flatnonzero(m.leaf).tolist() == [cap - 1]
    elif name == "one_per_block":
        for b in range(rp.sizes[1]):
            n = min(63, cap - (64 * b + 1))
            if n > 0:
                rp._zero_range(64 * b + 1, n)
        m.zero(np.flatnonzero(np.arange(cap) % 64))
        assert np.array_equal(np.flatnonzero(m.leaf), 64 * np.arange(rp.sizes[1]))
    elif name == "middle_subtree":
        K = cap // 2                               # a wrapped insert moves the oldest slot to the middle
        drv.apply(("insert", {k: v[:K] for k, v in first[1].items()}, first[2][:K]))
        n = 192 if cap < 100_000 else 8192
        drv.apply(("evict", n))
        dead = np.flatnonzero(m.leaf == 0)
        assert dead.tolist() == list(range(K, K + n)) and K % 64 == 0
        lv = m.levels()
        assert np.count_nonzero(lv[1] == 0) == n // 64 and (cap < 100_000 or np.count_nonzero(lv[2] == 0) == 1)
    elif name == "second_half":
        drv.apply(("evict", cap // 2))
        assert np.flatnonzero(m.leaf)[0] == cap // 2
    return rp, m


@pytest.mark.parametrize("name", ["leaf0", "last_leaf", "one_per_block", "middle_subtree", "second_half"])
@pytest.mark.parametrize("cap", [4097, BIG])
def test_sample_with_holes(cap, name):
    """512 draws over trees that are mostly empty: every row on a live leaf that owns its draw."""
    rp, m = _layout(cap, name)
    leaf = check_tree(rp, m)
    for ctr in (0, 7):
        rp.ctr.fill_(ctr)
        out = rp.sample(512)
        torch.cuda.synchronize()
        check_sample(rp, m, 512, out, leaf, ctr)
        assert np.all(out["weights"].cpu().numpy() > 0)


@pytest.mark.parametrize("cap", [4097, BIG])
def test_sample_from_an_empty_tree(cap):
    """No mass anywhere (never written, and written then evicted): the descent falls back to
    child 0 at every level and the leaf index is clamped, so every row reads slot [0, cap) and
    carries weight 0."""
    rp, m = _pair(cap)
    for emptied in (False, True):
        if emptied:
            drv = Driver(rp, m)
            first = next(random_ops(np.random.default_rng(4), cap, 1))
            drv.apply(first)
            drv.apply(("evict", len(first[2])))
            leaf = check_tree(rp, m)
            assert not np.any(leaf > 0)
        out = rp.sample(512)
        torch.cuda.synchronize()
        idx = out["idx"].cpu().numpy()
        assert np.all((idx >= 0) & (idx < cap))
        assert np.all(out["weights"].cpu().numpy() == 0)
        np.testing.assert_array_equal(out["act"].cpu().numpy(), m.act[idx])


# --------------------------------------------------------- 5. update limits
def _update(rp, m, idx, td, gen=None, **kw):
    idx, td = np.asarray(idx, np.int64), np.asarray(td, np.float32)
    gen = m.gen[idx] if gen is None else np.asarray(gen, np.int32)
    rp.update_priorities(_dev(idx), _dev(td), _dev(gen), **kw)
    return m.update(idx, td, gen)


def test_update_batch_sizes_and_counter():
    """n in {1, 63, 65, 1024} on the two-tier tree (one block of ceil(n / 64) waves); the sampling
    counter advances by exactly one per call when ``bump_ctr`` is set -- also when every row is
    stale -- and not at all otherwise."""
    rp, m, _ = _filled(BIG)
    rng = np.random.default_rng(5)
    live = BIG - 1500
    ctr = 0
    for n in (1, 63, 65, 1024):
        idx = rng.integers(0, live, n)
        if n > 4:
            idx[[0, n - 1]] = idx[n // 2]
        _update(rp, m, idx, rng.random(n) * 4)
        ctr += 1
        check_tree(rp, m)
        assert int(rp.ctr.item()) == ctr
    before = rp.leaf.clone(), rp.nodes.clone()
    idx = rng.integers(0, live, 65)
    win = _update(rp, m, idx, rng.random(65), m.gen[idx] + 1)           # every row stale
    torch.cuda.synchronize()
    assert win.size == 0 and int(rp.ctr.item()) == ctr + 1
    assert torch.equal(rp.leaf, before[0]) and torch.equal(rp.nodes, before[1])
    _update(rp, m, idx, rng.random(65), bump_ctr=False)
    check_tree(rp, m)
    assert int(rp.ctr.item()) == ctr + 1


def test_update_1024_rows_on_one_leaf_last_wins():
    rp, m, _ = _filled(BIG)
    td = (np.random.default_rng(6).random(1024) * 4 + 0.1).astype(np.float32)
    s = 64 * 4000 - 7
    win = _update(rp, m, np.full(1024, s), td)
    leaf = check_tree(rp, m)
    assert win.tolist() == [1023] and m.touch[1].sum() == (BIG - 1500) + 1
    np.testing.assert_allclose(leaf[s], m.prio_leaf(td[1023:])[0], rtol=2e-6)
    assert leaf[s] != m.prio_leaf(td[1022:1023])[0]


@pytest.mark.parametrize("spread", ["packed", "one_per_parent"])
def test_update_1024_distinct_leaves_atomic_path(spread):
    """Level 1 of the two-tier tree takes one global atomic per leaf.  ``packed``: 1024 adjacent
    leaves, i.e. 16 level-1 parents with all 64 children written (a level-1 node has only 64
    children, so 1024 distinct leaves cannot share one; they share one level-2 parent) -- the
    most atomics one node can see; ``one_per_parent``: 1024 different level-1 parents."""
    rp, m, _ = _filled(BIG)
    rng = np.random.default_rng(8)
    idx = 4096 * 3 + 64 * 5 + np.arange(1024) if spread == "packed" else 64 * rng.permutation(4000)[:1024] + 63
    idx = rng.permutation(idx)
    t0 = m.touch[1].copy()
    win = _update(rp, m, idx, rng.random(1024) * 4 + 0.05)
    assert win.size == 1024
    assert np.count_nonzero(m.touch[1] - t0) == (16 if spread == "packed" else 1024)
    check_tree(rp, m)


def test_update_over_1024_rows_is_refused_and_writes_nothing():
    rp, m, _ = _filled(BIG)
    torch.cuda.synchronize()
    before = rp.leaf.clone(), rp.nodes.clone(), rp.min_bits.clone()
    idx = torch.arange(1025, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="tree_update"):
        rp.update_priorities(idx, torch.ones(1025, device=DEV), rp.gen[idx].clone())
    torch.cuda.synchronize()
    assert torch.equal(rp.leaf, before[0]) and torch.equal(rp.nodes, before[1]) and torch.equal(rp.min_bits, before[2])
    assert int(rp.ctr.item()) == 0
    check_tree(rp, m)


# ---------------------------------------------------- 6. fused write-backs
@pytest.mark.parametrize("B", [64, 1024])
@pytest.mark.parametrize("route", ["head_wgrad", "fc_head_wgrad"])
def test_fused_write_back_matches_stand_alone_update(route, B):
    """The priority write-back riding in the head weight-gradient launch (512-thread block) and in
    the fc + head weight-gradient launch (256 threads: four item rounds at B = 1024) on the
    two-tier tree: leaves bit-equal to a stand-alone update_priorities of the same rows on a copy
    of the state, both trees within the model's bound at every level, and ``stats_out`` (the
    shard's slot of the all-gathered statistics) equal to the root and the minimum afterwards."""
    from apex_dqn_amd.ops.fused_ops import HipBackend
    rp, m, _ = _filled(BIG)
    rp.enable_sharding(0, 1, 3)
    ref = _clone(rp)
    rng = np.random.default_rng(B)
    live = BIG - 1500
    idx = rng.integers(0, live, B).astype(np.int64)
    idx[B // 2:B // 2 + 8] = idx[0]                       # duplicates of row 0's leaf: the last valid one wins
    idx[5:9] = BIG - 1 - np.arange(4)                     # never-written slots
    gen = m.gen[idx].copy()
    gen[B // 2 + 7] = -1                                  # a foreign row as the last duplicate
    gen[10:14] += 1                                       # stale
    gen[B - 3:] = -1                                      # foreign rows ...
    idx[B - 3:] = idx[1]                                  # ... on a leaf a valid row drew earlier
    td = (rng.random(B) * 4 + 0.01).astype(np.float32)
    A = 4
    g = torch.Generator(device="cpu").manual_seed(B)
    H = torch.rand(B, 1024, generator=g).to(DEV, torch.bfloat16)
    dhead = (torch.randn(B, A + 1, generator=g) * 1e-3).to(DEV)
    gh = {"wv": torch.zeros(512, device=DEV), "bv": torch.zeros(1, device=DEV),
          "wa": torch.zeros(A, 512, device=DEV), "ba": torch.zeros(A, device=DEV)}
    prio = (rp, _dev(idx), _dev(gen), _dev(td))
    be = HipBackend()
    if route == "head_wgrad":
        be.head_wgrad(H, dhead, gh, prio=prio)
    else:
        dH = (torch.randn(B, 1024, generator=g) * 0.01).to(DEV, torch.bfloat16)
        y3 = torch.relu(torch.randn(B, 3136, generator=g)).to(DEV, torch.bfloat16)
        gw, gb = torch.zeros(1024, 3136, device=DEV), torch.zeros(1024, device=DEV)
        part = torch.zeros(4096, dtype=torch.float64, device=DEV)
        assert be.fc_head_wgrad(dH, y3, gw, gb, H, dhead, gh, prio, norm=(part, 0)) > 0
    ref.update_priorities(prio[1], prio[3], prio[2])
    win = m.update(idx, td, gen)
    assert 0 < win.size < B - 12
    check_tree(rp, m)
    check_tree(ref, m)
    assert torch.equal(rp.leaf, ref.leaf) and torch.equal(rp.min_bits, ref.min_bits)
    assert int(rp.ctr.item()) == int(ref.ctr.item()) == 1
    st = rp.local_stats.cpu().numpy()
    assert st[0] == rp.total() and st[1] == rp.min_leaf()
    assert float(gh["wv"].abs().sum()) > 0


# ------------------------------------------------------- 7. sharded draw
_SHARDS = []


def _shards():
    """Three two-tier shards, read-only: 20 000 live leaves, none, and 256 549."""
    if not _SHARDS:
        for r, K in enumerate((20_000, 0, BIG - 1500)):
            rp, m = _pair(BIG, seed=20 + r)
            if K:
                first = next(random_ops(np.random.default_rng(30 + r), BIG, 1))
                Driver(rp, m).apply(("insert", {k: v[:K] for k, v in first[1].items()}, first[2][:K]))
            _SHARDS.append((rp, m, check_tree(rp, m)))
    return _SHARDS


@pytest.mark.parametrize("ranks,B,mcap", [((0, 1, 2), 64, 0), ((0, 1, 2), 3, 0), ((0, 1, 2), 64, 40),
                                          ((2, 1, 0), 512, 0), ((2,), 64, 0)])
def test_sharded_draw_partitions_the_strata(ranks, B, mcap):
    """One global stratified draw over shards of very unequal mass, one of them empty: the
    ranks' valid rows are a prefix of each batch and together take the strata 0 .. M - 1 once
    each, in rank order; stratum j's draw (j + U_j) * delta -- recomputed here in plain Python
    floats -- lies in the owning rank's mass interval and on the sampled leaf; an empty shard
    returns only invalid rows (weight 0, generation -1).  Also W == 1, B == 3 and a global batch
    capped below W * B."""
    sh = [_shards()[r] for r in ranks]
    W, seed, ctr = len(sh), 0xABCDEF, 2 ** 33 + 5
    T = [rp.total() for rp, _, _ in sh]
    sm, tmax, pmin = 0.0, 0.0, math.inf
    for (rp, _, _), t in zip(sh, T):
        sm += t
        tmax = max(tmax, t)
        if t > 0:
            pmin = min(pmin, float(np.float32(rp.min_leaf())))
    mb = B if W == 1 else math.floor((B - 2) * sm / tmax)
    M = int(min(mcap if mcap > 0 else W * B, max(mb, 0)))
    assert 0 < M and (mcap == 0 or M == mcap)
    delta = sm / M
    stats = torch.tensor([[t, rp.min_leaf() if t > 0 else 0.0, 0.0] for (rp, _, _), t in zip(sh, T)],
                         dtype=torch.float64)
    j_next, c0 = 0, 0.0
    for r, (rp, m, leaf) in enumerate(sh):
        rp.enable_sharding(r, W, seed, mcap=mcap)
        try:
            rp.shard_stats.copy_(stats.reshape(-1))
            rp.ctr.fill_(ctr)
            out = rp.sample(B)
            torch.cuda.synchronize()
        finally:
            rp.shard_stats = rp.local_stats = None
            rp.shard_rank, rp.shard_world, rp.shard_mcap = 0, 1, 0
        gen, idx, w = (out[k].cpu().numpy() for k in ("gen", "idx", "weights"))
        valid = gen >= 0
        nv = int(valid.sum())
        assert valid[:nv].all() and np.all(gen[nv:] == -1) and np.all(w[nv:] == 0)
        assert np.all((idx >= 0) & (idx < rp.cap))
        c1 = c0 + T[r]
        if T[r] == 0:
            assert nv == 0
        js = range(j_next, j_next + nv)
        uj = np.array([(float(j) + float(apex_uniform(seed, ctr, j))) * delta for j in js], np.float64)
        assert np.all(uj >= c0) and (r == W - 1 or np.all(uj < c1)), (r, j_next, nv)
        if r < W - 1 and j_next + nv < M:          # the next stratum's draw is not this rank's
            assert (float(j_next + nv) + float(apex_uniform(seed, ctr, j_next + nv))) * delta >= c1
        if nv:
            check_exact_draw(leaf, idx[:nv], np.clip(uj - c0, 0.0, T[r]), T[r])
            want = np.minimum((leaf[idx[:nv]].astype(np.float64) / pmin) ** -rp.beta, 1.0) * np.float32(W * B / M)
            np.testing.assert_allclose(w[:nv], want, rtol=1e-5)
            np.testing.assert_array_equal(gen[:nv], m.gen[idx[:nv]])
            np.testing.assert_array_equal(out["obs"].cpu().numpy()[:nv], m.obs[idx[:nv]])
        j_next += nv
        c0 = c1
    assert j_next == M


def test_sharded_draw_of_two_rows_is_refused():
    """``shard_stats`` set and B = 2 (an interval catches up to floor(T M / sum) + 2 strata, so a sharded
    draw needs B >= 3): ``sample`` refuses, and so does the launcher when handed the block; nothing is drawn."""
    rp, _, _ = _filled(64)
    rp.enable_sharding(0, 1, 3)
    out = rp.alloc_sample_buffers(2)
    out["idx"].fill_(-1)
    with pytest.raises(ValueError, match="B >= 3"):
        rp.sample(2, out=out)
    assert rp.lib.apex_tree_sample(rp.sample_launch_args(2, out), rp._stream()) == 1
    torch.cuda.synchronize()
    assert bool((out["idx"] == -1).all())
    assert rp.lib.apex_tree_sample(rp.sample_launch_args(3, rp.alloc_sample_buffers(3)), rp._stream()) == 0
    torch.cuda.synchronize()
