"""Host side of the float32 neck's polyphase launch (depth.py neck_poly_compose, csrc/vd3d_conv_poly.hip): the composition is the module chain in float64, the
multiply-add count it leaves, the refusals, the restated weight image, and the C boundary.  No GPU needed."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from visiondepth3d_amd import _abi, _lib
from visiondepth3d_amd.depth import neck_poly_compose, neck_poly_offsets

BUILT = ((96, 128, 4), (192, 128, 2), (48, 64, 4), (96, 64, 2))
MAPS = ((1, 1), (1, 5), (5, 1), (2, 1), (5, 7))


def poly_eval(x, Wc, bc, f):
    """The composed form with plain torch ops, in the dtype of its operands: per block one matrix product over the shifted coarse map, zero outside the map, the
    block's bias wherever its coarse pixel is inside."""
    B, _, h, w = x.shape
    out = x.new_zeros(B, Wc.shape[1], f * h, f * w)
    xp = F.pad(x, (1, 1, 1, 1))
    inside = F.pad(x.new_ones(1, 1, h, w), (1, 1, 1, 1))
    for k, (pa, pb, di, dj) in enumerate(neck_poly_offsets(f)):
        xs, ins = xp[:, :, 1 + di:1 + di + h, 1 + dj:1 + dj + w], inside[:, :, 1 + di:1 + di + h, 1 + dj:1 + dj + w]
        out[:, :, pa::f, pb::f] += torch.einsum("oc,bchw->bohw", Wc[k], xs) + bc[k].view(1, -1, 1, 1) * ins
    return out


def pack_restated(Wc):
    """vd3d_neck_poly_pack_f32's image restated: [block][Cout][Cin] -> [block][slot Cin / KS][step KS / 8][k-half 2][oc Cout][4 floats], KS = 32 (16 where Cin is
    no multiple of 32), channel slot * KS + k-half * KS / 2 + 4 * step + e."""
    nblk, Cout, Cin = Wc.shape
    ks = 32 if Cin % 32 == 0 else 16
    return Wc.reshape(nblk, Cout, Cin // ks, 2, ks // 8, 4).permute(0, 2, 4, 3, 1, 5).contiguous().reshape(-1)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.mark.parametrize("f", (4, 2))
@pytest.mark.parametrize("hw", MAPS, ids=["%dx%d" % m for m in MAPS])
def test_composition_is_the_module_chain_in_float64(f, hw):
    g = torch.Generator().manual_seed(100 * f + 10 * hw[0] + hw[1])
    Cin, C, Cout = 6, 5, 7
    wt = torch.randn(Cin, C, f, f, generator=g, dtype=torch.float64)
    bt = torch.randn(C, generator=g, dtype=torch.float64)
    w3 = torch.randn(Cout, C, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(3, Cin, *hw, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.conv_transpose2d(x, wt, bt, stride=f), w3, None, padding=1)
    Wc, bc = neck_poly_compose(wt, bt, w3, f, dtype=torch.float64)
    assert Wc.shape == ((f + 2) ** 2, Cout, Cin) and bc.shape == ((f + 2) ** 2, Cout)
    got = poly_eval(x, Wc, bc, f)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # without a bias: the same with zero bias blocks
    Wn, bn = neck_poly_compose(wt, None, w3, f, dtype=torch.float64)
    assert torch.equal(Wn, Wc) and not bool(bn.any())
    # the float32 result is the float64 one rounded once
    W32, b32 = neck_poly_compose(wt.float(), bt.float(), w3.float(), f)
    W64, b64 = neck_poly_compose(wt.float(), bt.float(), w3.float(), f, dtype=torch.float64)
    assert W32.dtype == torch.float32 and torch.equal(W32, W64.float()) and torch.equal(b32, b64.float())


def test_blocks_and_multiply_adds_per_output_pixel():
    """(f + 2)^2 blocks in the stated order; DA-V2-Base: 96 channels x 36 blocks / 16 phases = 216 multiply-adds per output pixel and channel (the module chain:
    96 + 9 x 96 = 960, of which the 3 x 3 convolution's 864), 192 x 16 / 4 = 768 (192 + 1728)."""
    o4, o2 = neck_poly_offsets(4), neck_poly_offsets(2)
    assert len(o4) == 36 and len(o2) == 16
    assert len(o4) * 96 // 16 == 216 and len(o2) * 192 // 4 == 768
    assert o2 == [(pa, pb, di, dj) for pa in (0, 1) for pb in (0, 1) for di in ((-1, 0), (0, 1))[pa] for dj in ((-1, 0), (0, 1))[pb]]
    assert o4[:4] == [(0, 0, -1, -1), (0, 0, -1, 0), (0, 0, 0, -1), (0, 0, 0, 0)] and o4[4:6] == [(0, 1, -1, 0), (0, 1, 0, 0)] and o4[-1] == (3, 3, 1, 1)
    assert o4 == sorted(o4) and o2 == sorted(o2)
    assert [sum(1 for o in o4 if o[:2] == (pa, pb)) for pa in range(4) for pb in range(4)] == [4, 2, 2, 4, 2, 1, 1, 2, 2, 1, 1, 2, 4, 2, 2, 4]


def test_wrong_argument_shapes_are_refused():
    wt, bt, w3 = torch.zeros(6, 5, 4, 4), torch.zeros(5), torch.zeros(7, 5, 3, 3)
    neck_poly_compose(wt, bt, w3, 4)
    for bad in ((wt, bt, w3, 2),                              # the factor is not the kernel size
                (torch.zeros(6, 5, 4, 2), bt, w3, 4),
                (wt, torch.zeros(6), w3, 4),                  # the bias belongs to the transposed convolution's OUTPUT channels
                (wt, bt, torch.zeros(7, 6, 3, 3), 4),         # the 3 x 3 convolution reads those channels
                (wt, bt, torch.zeros(7, 5, 1, 1), 4),
                (wt[0], bt, w3, 4)):
        with pytest.raises(ValueError):
            neck_poly_compose(*bad)
    for f in (1, 0, 2.5):
        with pytest.raises(ValueError):
            neck_poly_offsets(f)


def test_weight_image_layout_round_trips():
    """The restated layout against the index the kernel reads with: the A fragment of (step, k-half, oc) sits at ((step * 2 + k-half) * Cout + oc) * 4 floats inside a
    slot of KS / 8 * 2 * Cout * 4 floats."""
    for Cin, Cout, f in BUILT:
        nblk = (f + 2) ** 2
        Wc = torch.arange(nblk * Cout * Cin, dtype=torch.float32).reshape(nblk, Cout, Cin)
        img = pack_restated(Wc)
        ks = 32 if Cin % 32 == 0 else 16
        slot = ks // 8 * 2 * Cout * 4
        g = torch.Generator().manual_seed(Cin + Cout)
        for _ in range(200):
            k, oc, ci = (int(torch.randint(n, (1,), generator=g)) for n in (nblk, Cout, Cin))
            s, r = divmod(ci, ks)
            khalf, r = divmod(r, ks // 2)
            st, e = divmod(r, 4)
            assert float(img[(k * (Cin // ks) + s) * slot + ((st * 2 + khalf) * Cout + oc) * 4 + e]) == float(Wc[k, oc, ci])


def test_c_boundary(L):
    hdr = open(os.path.join(ROOT, "include", "vd3d.h")).read()
    declared = set(re.findall(r"\b(vd3d_[a-z0-9_]+)\s*\(", hdr))
    new = {"vd3d_neck_poly_weight_bytes", "vd3d_neck_poly_pack_f32", "vd3d_neck_poly_conv_f32"}
    assert new <= declared and new <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    for n in new:
        assert hasattr(L, n), n
        assert re.search(r"Additions since 6 that leave the version as it is.*?" + n + r".*?\*/\s*#define VD3D_ABI_VERSION 6", hdr, re.S)
    assert _abi.ABI_VERSION == 6 and L.vd3d_abi_version() == 6
    for Cin in (48, 64, 96, 192, 256):
        for Cout in (64, 128, 256):
            for f in (1, 2, 3, 4):
                nb = L.vd3d_neck_poly_weight_bytes(Cin, Cout, f)
                assert nb == ((f + 2) ** 2 * Cout * Cin * 4 if (Cin, Cout, f) in BUILT else -1), (Cin, Cout, f, nb)
    # pure host refusals: no context is needed to be told that an argument is missing
    assert L.vd3d_neck_poly_pack_f32(None, None, 96, 128, 4, None) == _abi.E_INVALID
    assert L.vd3d_neck_poly_conv_f32(None, None, 1, 5, 7, 96, None, None, 128, 4, None) == _abi.E_INVALID
