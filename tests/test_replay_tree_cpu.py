"""A plain numpy fp64 model of the prioritized-replay shard (csrc/sumtree.hip semantics: 64-ary
sum-tree over fp32 leaves, record ring, slot generations) and the CPU tests that validate it
against ``GpuReplayShard(device="cpu")``.  tests/test_gpu_replay_tree.py then holds the HIP
kernels to the same model, so the model shares no code with either replay path.

Running minimum: the torch path recomputes the minimum over the positive leaves on every
mutation, so ``min_leaf()`` is exact there.  The kernels keep a running ``atomicMin`` of every
positive value written since the last rebuild, which is only a LOWER bound of the true minimum
once the minimum leaf was overwritten with a larger value or evicted; ``rebuild()`` makes it
exact again (:class:`TreeModel` tracks ``min_stale`` for that)."""
import math

import numpy as np
import pytest
import torch

from apex_dqn_amd.replay.gpu_replay import GpuReplayShard, apex_uniform

FOREIGN = -(1 << 20)      # generation offset marking a row of another shard (gen_expect = -1)
TREE_LACC = 4096          # csrc/sumtree.hip: LDS accumulator entries of tree_block_update
U52, U53 = 2.0 ** -52, 2.0 ** -53


def tree_sizes(cap):
    sizes = [int(cap)]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + 63) // 64)
    return sizes


def kfirst(sizes):
    """Mirror of csrc/sumtree.hip ``tree_kfirst``: the lowest level that, together with every
    level above it, holds at most TREE_LACC nodes (levels below it take per-leaf atomics)."""
    L = len(sizes) - 1
    k, s = L, sizes[L]
    while k > 1 and s + sizes[k - 1] <= TREE_LACC:
        s += sizes[k - 1]
        k -= 1
    return k


class TreeModel:
    """Host oracle of one replay shard.  Leaves are float32((|p| + eps) ** alpha) computed in
    fp64; ``levels`` sums them exactly.  For the fp64-delta kernels it also tracks, per internal
    node, ``touch`` (the deltas that reached the node since the last rebuild) and ``peak`` (the
    largest value the node held after any op since then): every delta costs the node at most one
    rounding of the delta and one of the accumulation, each <= 2**-53 of the values involved, so
    ``touch * 2**-52 * peak`` bounds the drift."""

    def __init__(self, cap, C, alpha=0.6, eps=1e-6):
        self.cap, self.C, self.alpha, self.eps = int(cap), int(C), float(alpha), float(eps)
        self.sizes = tree_sizes(cap)
        self.L = len(self.sizes) - 1
        self.leaf = np.zeros(cap, np.float32)
        self.gen = np.zeros(cap, np.int32)
        self.obs = np.zeros((cap, C), np.int32)
        self.nxt = np.zeros((cap, C), np.int32)
        self.act = np.zeros(cap, np.int32)
        self.rew = np.zeros(cap, np.float32)
        self.gam = np.zeros(cap, np.float32)
        self.touch = [None] + [np.zeros(n, np.int64) for n in self.sizes[1:]]
        self.peak = [None] + [np.zeros(n, np.float64) for n in self.sizes[1:]]
        self.min_stale = False

    # ---------------------------------------------------------------- values
    def prio_leaf(self, p):
        p = np.abs(np.asarray(p, np.float32).astype(np.float64))
        return ((p + self.eps) ** self.alpha).astype(np.float32)

    def levels(self, leaf=None):
        """[leaf fp64, level 1, ..., root]: exact sums of 64 children per parent (accumulated in
        extended precision where the platform has it, rounded to fp64 once per node)."""
        leaf = self.leaf if leaf is None else leaf
        prev = np.asarray(leaf).astype(np.longdouble)
        out = [prev.astype(np.float64)]
        for n in self.sizes[1:]:
            pad = np.zeros(n * 64, np.longdouble)
            pad[:prev.size] = prev
            prev = pad.reshape(n, 64).sum(1)
            out.append(prev.astype(np.float64))
        return out

    def true_min(self, leaf=None):
        leaf = self.leaf if leaf is None else np.asarray(leaf)
        pos = leaf[leaf > 0]
        return float(pos.min()) if pos.size else math.inf

    def locate(self, u, leaf=None):
        leaf = self.leaf if leaf is None else leaf
        c = np.cumsum(np.asarray(leaf).astype(np.float64))
        return np.minimum(np.searchsorted(c, np.asarray(u, np.float64), side="right"), self.cap - 1)

    @staticmethod
    def draws(B, seed, ctr, total):
        b = np.arange(B)
        return (b + apex_uniform(seed, ctr, b).astype(np.float64)) * (float(total) / B)

    # ------------------------------------------------------------- mutations
    def _write(self, slots, vals):
        slots = np.asarray(slots, np.int64)
        vals = np.asarray(vals, np.float32)
        m0 = self.true_min()
        moved = self.leaf[slots] != vals
        self.leaf[slots] = vals
        for k in range(1, self.L + 1):
            self.touch[k] += np.bincount(slots[moved] >> (6 * k), minlength=self.sizes[k])
        self._note_peak()
        if self.true_min() > m0:      # the minimum leaf was raised or removed
            self.min_stale = True

    def _note_peak(self):
        for k, lv in enumerate(self.levels()):
            if k:
                np.maximum(self.peak[k], lv, out=self.peak[k])

    def insert(self, start, records, prio):
        K = len(prio)
        slots = (int(start) + np.arange(K)) % self.cap
        for name in ("obs", "nxt", "act", "rew", "gam"):
            getattr(self, name)[slots] = records[name]
        self.gen[slots] += 1
        self._write(slots, self.prio_leaf(prio))
        return slots

    def update(self, idx, td, gen_expect=None):
        idx = np.asarray(idx, np.int64)
        td = np.asarray(td, np.float32)
        rows = np.arange(idx.size)
        if gen_expect is not None:
            gen_expect = np.asarray(gen_expect, np.int32)
            rows = rows[gen_expect >= 0]
        last = {}
        for i in rows:                # the last remaining occurrence of an index wins
            last[int(idx[i])] = int(i)
        win = np.array(sorted(last.values()), np.int64)
        if win.size:
            s = idx[win]
            ok = self.leaf[s] > 0
            if gen_expect is not None:
                ok &= self.gen[s] == gen_expect[win]
            win = win[ok]
        self._write(idx[win], self.prio_leaf(td[win]))
        return win

    def zero_range(self, start, count):
        self.zero((int(start) + np.arange(int(count))) % self.cap)

    def zero(self, slots):
        self._write(slots, np.zeros(len(slots), np.float32))

    def rebuilt(self):
        """rebuild() ran: the nodes and the minimum are exact again."""
        for k in range(1, self.L + 1):
            self.touch[k][:] = 0
            self.peak[k][:] = 0
        self._note_peak()
        self.min_stale = False

    def node_bound(self, k):
        """Largest |node - exact sum| the kernels may leave at level k: the delta drift plus what
        an exact rebuild leaves (k levels of 64-term sums, summation order only)."""
        return self.touch[k] * U52 * self.peak[k] + k * 64 * U53 * self.peak[k]


def random_ops(rng, cap, n_ops, C=4, F=64, max_insert=3000):
    """A seeded op sequence: ("insert", records, prio) / ("update", idx, td, gen_offset) /
    ("evict", n) / ("sample", B) / ("rebuild",).  The first op fills most of the ring so that
    the following inserts wrap it over live leaves.  Updates hold at most 1024 rows with
    duplicates, stale generations (offset +-1), rows on evicted or never-written slots (indices
    are drawn over the whole ring) and FOREIGN rows (gen_expect = -1)."""
    head = live = 0

    def insert(K):
        nonlocal head, live
        rec = dict(obs=rng.integers(0, F, (K, C)).astype(np.int32), nxt=rng.integers(0, F, (K, C)).astype(np.int32),
                   act=rng.integers(0, 18, K).astype(np.int32), rew=rng.normal(size=K).astype(np.float32),
                   gam=np.where(rng.random(K) < 0.1, 0.0, 0.97).astype(np.float32))
        prio = (rng.random(K) * 3 + 0.01).astype(np.float32) * rng.choice([1.0, -1.0], K).astype(np.float32)
        head, live = (head + K) % cap, min(live + K, cap)
        return ("insert", rec, prio)

    yield insert(cap - min(cap // 4, 1500))
    for i in range(1, n_ops):
        r = rng.random()
        if i in (1, 2) or r < 0.3:
            yield insert(int(rng.integers(1, min(cap, max_insert) + 1)))
        elif r < 0.6:
            n = int(rng.choice([1, 63, 64, 65, 700, 1024]))
            idx = rng.integers(0, cap, n)
            if n > 4:                 # duplicates: three rows on one leaf, a run on another
                idx[[0, n // 2, n - 1]] = idx[1]
                idx[2:2 + n // 8] = idx[3]
            off = rng.choice([0, 0, 0, 0, 0, 1, -1, FOREIGN], n).astype(np.int64)
            yield ("update", idx.astype(np.int64), (rng.random(n) * 5).astype(np.float32), off)
        elif r < 0.75 and live > 1:
            n = int(rng.integers(1, max(2, min(live, 2 * max_insert))))
            live -= n
            yield ("evict", n)
        elif r < 0.92:
            yield ("sample", int(rng.choice([1, 3, 64, 257])))
        else:
            yield ("rebuild",)


class Driver:
    """Applies one op to a GpuReplayShard and to the model, tracking the ring head itself."""

    def __init__(self, rp, model):
        self.rp, self.m = rp, model
        self.head = self.live = 0
        self.last_sample = None

    def apply(self, op):
        rp, m, dev = self.rp, self.m, self.rp.device
        if op[0] == "insert":
            rec, prio = op[1], op[2]
            K = len(prio)
            slots = rp.insert(dict(S_t=rec["obs"], S_tpn=rec["nxt"], A_t=rec["act"], R=rec["rew"], Gamma=rec["gam"],
                                   priority=prio))
            ms = m.insert(self.head, rec, prio)
            np.testing.assert_array_equal(slots, ms)
            self.head, self.live = (self.head + K) % m.cap, min(self.live + K, m.cap)
        elif op[0] == "update":
            idx, td, off = op[1], op[2], op[3]
            gen = np.where(off == FOREIGN, -1, m.gen[idx].astype(np.int64) + off).astype(np.int32)
            rp.update_priorities(torch.from_numpy(idx).to(dev), torch.from_numpy(td).to(dev),
                                 torch.from_numpy(gen).to(dev))
            m.update(idx, td, gen)
        elif op[0] == "evict":
            n = op[1]
            soft, rp.soft_capacity = rp.soft_capacity, self.live - n
            assert rp.remove_to_fit() == n
            rp.soft_capacity = soft
            m.zero_range((self.head - self.live) % m.cap, n)
            self.live -= n
        elif op[0] == "sample":
            self.last_sample = (op[1], rp.sample(op[1]))
        elif op[0] == "rebuild":
            rp.rebuild()
            m.rebuilt()
        assert rp.size() == self.live and rp.head == self.head


def check_exact_draw(leaf, idx, u, total):
    """Every row's leaf is live and owns its draw: c[i] - leaf[i] <= u < c[i], up to 1e-9 of the
    total (the margin test_sharded_sample_hip_matches_global_draw uses)."""
    leaf = np.asarray(leaf).astype(np.float64)
    c = np.cumsum(leaf)
    tol = 1e-9 * float(total)
    assert np.all(leaf[idx] > 0), np.flatnonzero(leaf[idx] <= 0)
    lo_ok, hi_ok = c[idx] - leaf[idx] <= u + tol, u < c[idx] + tol
    assert np.all(lo_ok) and np.all(hi_ok), (np.flatnonzero(~lo_ok), np.flatnonzero(~hi_ok))


def check_records(rp, m):
    for name in ("gen", "act", "rew", "gam", "obs", "nxt"):
        np.testing.assert_array_equal(getattr(rp, name).cpu().numpy(), getattr(m, name), err_msg=name)


def check_sample(rp, m, B, out, leaf, ctr):
    """An unsharded ``sample(B)`` output against the reconstructed draws u_b."""
    total = float(rp.nodes[rp.offs[rp.L]].item())
    idx = out["idx"].cpu().numpy()
    w = out["weights"].cpu().numpy()
    assert np.all((idx >= 0) & (idx < m.cap))
    if not np.any(leaf > 0):
        assert np.all(w == 0)
        return
    check_exact_draw(leaf, idx, m.draws(B, rp.seed, ctr, total), total)
    pmin = np.float64(rp.min_leaf())
    np.testing.assert_allclose(w, np.minimum((leaf[idx].astype(np.float64) / pmin) ** -rp.beta, 1.0), rtol=1e-5)
    for name in ("gen", "act", "rew", "gam", "obs", "nxt"):
        np.testing.assert_array_equal(out[name].cpu().numpy(), getattr(m, name)[idx], err_msg=name)


# ------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("cap", [64, 65, 1000, 4097])
def test_cpu_shard_follows_the_model(cap):
    """The torch path recomputes every node and the minimum exactly after each mutation: leaves
    at rtol 2e-6, records and generations bit-equal, every level equal to the exact sums of the
    shard's own leaves (summation order only), min_leaf() the exact minimum."""
    rp = GpuReplayShard(cap, cap, 64, 4, device="cpu", seed=5)
    m = TreeModel(cap, 4, rp.alpha, rp.eps)
    drv = Driver(rp, m)
    kinds = set()
    wrapped = False
    for op in random_ops(np.random.default_rng(cap), cap, 40, max_insert=1500):
        h0 = drv.head
        drv.apply(op)
        kinds.add(op[0])
        wrapped |= op[0] == "insert" and drv.head <= h0
        leaf = rp.leaf.numpy()
        np.testing.assert_allclose(leaf, m.leaf, rtol=2e-6)
        np.testing.assert_array_equal(leaf > 0, m.leaf > 0)
        check_records(rp, m)
        for k, lv in enumerate(m.levels(leaf)):
            if k:
                got = rp.nodes[rp.offs[k]:rp.offs[k] + rp.sizes[k]].numpy()
                np.testing.assert_allclose(got, lv, rtol=k * 64 * U53, atol=0, err_msg=f"level {k}")
        assert rp.min_leaf() == m.true_min(leaf)
        if op[0] == "sample":
            B, out = drv.last_sample
            check_sample(rp, m, B, out, leaf, int(rp.ctr.item()))
            np.testing.assert_array_equal(np.sort(out["idx"].numpy()), out["idx"].numpy())
    assert kinds == {"insert", "update", "evict", "sample", "rebuild"} and wrapped
    assert int(rp.ctr.item()) > 0 and m.gen.max() >= 2


def test_model_update_semantics():
    """The model's dedupe: foreign rows are dropped first, then the last remaining occurrence
    wins, then an evicted leaf or a stale generation skips the row."""
    m = TreeModel(100, 1, alpha=1.0, eps=0.0)
    rec = dict(obs=np.zeros((10, 1), np.int32), nxt=np.zeros((10, 1), np.int32), act=np.zeros(10, np.int32),
               rew=np.zeros(10, np.float32), gam=np.zeros(10, np.float32))
    m.insert(95, rec, np.arange(1, 11, dtype=np.float32))            # slots 95..99, 0..4
    assert list(np.flatnonzero(m.leaf)) == [0, 1, 2, 3, 4, 95, 96, 97, 98, 99] and m.leaf[0] == 6.0
    m.zero_range(99, 2)                                              # slots 99 and 0
    assert m.leaf[99] == 0 and m.leaf[0] == 0 and m.min_stale is False and m.true_min() == 1.0
    win = m.update([1, 1, 2, 1, 0, 3], [5, 6, 7, 8, 9, 10], [1, 1, 1, -1, 1, 0])
    assert list(win) == [1, 2] and m.leaf[1] == 6.0 and m.leaf[2] == 7.0 and m.leaf[3] == 9.0
    m.update([95], [50.0])                                           # the minimum leaf is raised
    assert m.min_stale and m.true_min() == 2.0
    lv = m.levels()
    assert lv[1][0] == m.leaf[:64].astype(np.float64).sum() and lv[2][0] == m.leaf.astype(np.float64).sum()
    assert m.touch[1][0] == 8 and m.touch[1][1] == 7 and m.touch[2][0] == 15
    u = np.array([0.0, 5.99, 6.0, 1e9])
    assert list(m.locate(u)) == [1, 1, 2, 99]
    d = m.draws(4, 3, 9, 8.0)
    assert np.all((d >= 2.0 * np.arange(4)) & (d < 2.0 * np.arange(1, 5)))


def test_kfirst_thresholds():
    """tree_kfirst's arithmetic: the LDS accumulator is exactly full at 258 048 leaves."""
    assert tree_sizes(258_048) == [258_048, 4032, 63, 1] and sum(tree_sizes(258_048)[1:]) == TREE_LACC
    assert tree_sizes(258_049) == [258_049, 4033, 64, 1]
    assert kfirst(tree_sizes(64)) == 1 and kfirst(tree_sizes(4097)) == 1 and kfirst(tree_sizes(126_024)) == 1
    assert kfirst(tree_sizes(258_048)) == 1
    assert kfirst(tree_sizes(258_049)) == 2
    assert kfirst(tree_sizes(391_649)) == 2 and len(tree_sizes(391_649)) - 1 == 4
    assert kfirst(tree_sizes(2_097_152)) == 2
    assert kfirst(tree_sizes(3_126_024)) == 2 and len(tree_sizes(3_126_024)) - 1 == 4
    assert kfirst(tree_sizes(16_515_073)) == 3


def test_capacity_below_two_is_refused():
    """A one-leaf ring has no internal level (L == 0): nothing would ever write the root."""
    for cap in (1, 0):
        with pytest.raises(ValueError):
            GpuReplayShard(cap, cap, 8, 4, device="cpu")
    assert GpuReplayShard(2, 2, 8, 4, device="cpu").L == 1
