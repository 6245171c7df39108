"""Fused conv1 -> conv2 -> conv3 forward with y2 written only for the rows a backward reads
(csrc/conv12_fused.hip ``Conv12Desc::y2_n``).

With conv3 fused the kernel takes y2 from LDS, so rows >= ``y2_n`` skip the 12 (bf16: 6)
global y2 stores per wave and image.  The wait after conv1 counts those stores to let
them stay in flight past the barrier while still covering the next image's frame DMA:
an image whose predecessor skipped its stores must drain everything instead, or DMA
pieces are still landing when conv1 of the next image reads them -- a wrong y3 on the
images after the flip, which is what the byte comparisons below would show.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = 0x5A5A        # bf16 bit pattern pre-filled into every output


def _lib():
    from apex_dqn_amd.ops import _lib as L
    return L.require_kernels()


def _split(x32):
    x32 = x32.to(DEV, torch.float32)
    hi = x32.to(torch.bfloat16)
    return hi, (x32 - hi.float()).to(torch.bfloat16)


def _filled(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16)


@pytest.fixture(scope="module")
def problem():
    """One set of frames and weights (online + target) shared by every case."""
    from apex_dqn_amd.replay.gpu_replay import to_s2d
    g = torch.Generator(device="cpu").manual_seed(33)
    raw = torch.randint(0, 256, (40, 84, 84), generator=g, dtype=torch.uint8)
    p = {"ring": to_s2d(raw.to(DEV)),
         "slots": torch.randint(0, 40, (15, 4), generator=g, dtype=torch.int32).to(DEV)}
    for s in "ab":
        p["w1" + s] = (torch.randn(64, 4, 8, 8, generator=g) * 0.05).to(DEV)
        p["w2" + s] = torch.randn(64, 4, 4, 64, generator=g) * 0.03
        p["w3" + s] = torch.randn(64, 3, 3, 64, generator=g) * 0.04
        for k in "123":
            p["b" + k + s] = (torch.randn(64, generator=g) * 0.1).to(DEV)
    return p


def _run(p, N, Bs, grid, split, y2_n):
    from apex_dqn_amd.ops import conv as C_
    if split:
        (w2a, w2al), (w2b, w2bl) = _split(p["w2a"]), _split(p["w2b"])
        (w3a, w3al), (w3b, w3bl) = _split(p["w3a"]), _split(p["w3b"])
    else:
        w2a, w2b = p["w2a"].to(DEV, torch.bfloat16), p["w2b"].to(DEV, torch.bfloat16)
        w3a, w3b = p["w3a"].to(DEV, torch.bfloat16), p["w3b"].to(DEV, torch.bfloat16)
        w2al = w2bl = w3al = w3bl = None
    lo = (lambda *s: _filled(*s)) if split else (lambda *s: None)
    y1, y1l = _filled(Bs, 20, 20, 64), lo(Bs, 20, 20, 64)
    y2, y2l = _filled(N, 9, 9, 64), lo(N, 9, 9, 64)
    y3, y3l = _filled(N, 7, 7, 64), lo(N, 7, 7, 64)
    C_.conv12_fused_fwd(_lib(), C_.Workspace(), p["ring"], p["slots"][:N].contiguous(), p["w1a"], p["b1a"], w2a, w2al,
                        p["b2a"], 1 / 255.0, y2, y2l, y1=y1, y1_lo=y1l, copy_n=Bs, w1b=p["w1b"], b1b=p["b1b"],
                        w2b=w2b, w2b_lo=w2bl, b2b=p["b2b"], rows_first=2 * Bs, grid=grid,
                        c3=(w3a, w3al, p["b3a"], w3b, w3bl, p["b3b"]), y3=y3, y3_lo=y3l, y2_n=y2_n)
    torch.cuda.synchronize()
    return [t for t in (y1, y1l, y2, y2l, y3, y3l) if t is not None], 2 if split else 1


@pytest.mark.parametrize("split", [True, False], ids=["fp32", "bf16"])
@pytest.mark.parametrize("grid_all", [False, True], ids=["grid1", "gridN"])
@pytest.mark.parametrize("Bs", [2, 5])
def test_y2_rows_same_bytes_and_rest_untouched(problem, Bs, grid_all, split):
    """N = 3 Bs images (S_t, S_t+n online, S_t+n target from row 2 Bs), y2_n = Bs: y3 of every
    row, y1[:Bs] and y2[:Bs] are byte-equal to the launch that stores every row, and
    y2[Bs:] keeps its sentinel.  Grid 1: one workgroup crosses the flip and computes
    2 Bs >= 4 images after it; grid N: one image per workgroup."""
    N = 3 * Bs
    grid = N if grid_all else 1
    full, k = _run(problem, N, Bs, grid, split, None)
    part, _ = _run(problem, N, Bs, grid, split, Bs)
    y1f, y2f, y3f = full[:k], full[k:2 * k], full[2 * k:]
    y1p, y2p, y3p = part[:k], part[k:2 * k], part[2 * k:]
    for a in y2f + y3f + y1f:
        assert not (_bits(a) == SENTINEL).all(dim=-1).any()        # the all-rows launch wrote every pixel
    for a, b in zip(y3f, y3p):
        bad = (_bits(a) != _bits(b)).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"y3 differs on images {bad}"
    for a, b in zip(y1f, y1p):
        assert torch.equal(_bits(a), _bits(b))
    for a, b in zip(y2f, y2p):
        assert torch.equal(_bits(a[:Bs]), _bits(b[:Bs]))
        assert (_bits(b[Bs:]) == SENTINEL).all(), "a row >= y2_n was written"


def test_y2_rows_ignored_without_fused_conv3(problem):
    """Without the fused conv3 a separate launch reads y2: every row is stored whatever y2_n says."""
    from apex_dqn_amd.ops import conv as C_
    N, Bs = 6, 2
    (w2a, w2al), (w2b, w2bl) = _split(problem["w2a"]), _split(problem["w2b"])
    outs = []
    for y2_n in (None, Bs):
        y1, y1l = _filled(Bs, 20, 20, 64), _filled(Bs, 20, 20, 64)
        y2, y2l = _filled(N, 9, 9, 64), _filled(N, 9, 9, 64)
        C_.conv12_fused_fwd(_lib(), C_.Workspace(), problem["ring"], problem["slots"][:N].contiguous(), problem["w1a"],
                            problem["b1a"], w2a, w2al, problem["b2a"], 1 / 255.0, y2, y2l, y1=y1, y1_lo=y1l,
                            copy_n=Bs, w1b=problem["w1b"], b1b=problem["b1b"], w2b=w2b, w2b_lo=w2bl,
                            b2b=problem["b2b"], rows_first=2 * Bs, grid=1, y2_n=y2_n)
        torch.cuda.synchronize()
        outs.append((y2, y2l))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert not (_bits(outs[1][0]) == SENTINEL).all(dim=-1).any()
