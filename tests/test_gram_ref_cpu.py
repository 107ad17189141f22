"""The Gram tests' CPU helper (tests/_gram_ref.py) checked on its own: the
emulation is at rounding level, the exact kinds are exact as claimed, and the
check a GPU test applies (check()) rejects every planted fault.

Dropped product classes of the quad Gram, measured here (emulation with the
class left out, over the emulation's own measure; the check allows RATIO_MAX
= 4): on 3 parts an order-2 class 12 .. 26 on 'graded' and 'zeros', 26 .. 68
on 'late'; an order-1 class 8 000 .. 40 000; on 2 parts an order-1 class 300
.. 390.  So the measure does see a missing order-2 class, but by a factor of
3 to 5 over its bound, against an emulation whose 32-row blocks are exact;
the 'parts' kind sees it at 60 ulp against a bound of 1, whatever the
emulation does.  test_dropped_product_classes asserts the second and that the
first is above 1.
"""
import numpy as np
import pytest
import torch

import _gram_ref as G
from _apply_ref import RATIO_MAX, split_bf16

F32, F64 = torch.float32, torch.float64


def _rejected(case, C, np_=None):
    bad, _ = G.check(case, C, np_)
    return bool(bad)


# ------------------------------------------------------------- the helper
@pytest.mark.parametrize("shape", range(len(G.SHAPES)))
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("dtype,W", [(F32, 32), (F64, 64)])
def test_plain_emulation_is_at_rounding_level(dtype, W, kind, shape):
    rows = G.SHAPES[shape][2]
    for mode in ("full", "cross"):
        c = G.pair_case(kind, dtype, W, shape, mode)
        e = G.measure(c["emu"], c["ref"], c["den"])
        assert 0 < e < G.gamma_rows(dtype, rows), (mode, e)
        assert not _rejected(c, c["emu"])
    assert G.mirrored(G.pair_case(kind, dtype, W, shape, "full")["emu"], W)


@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("kind", G.KINDS)
def test_quad_emulation_is_at_rounding_level(kind, shape):
    """3 parts: the dropped products (2^-26) and the fp32 sums, below gamma of
    the chunk's rows; 2 parts: 3 x 2^-18 per product by design (the parts past
    the second and the product 1 x 1), below 2^-16."""
    c = G.quad_case(kind, 2, shape)
    e3 = G.measure(c["emu", 3], c["ref"], c["den"])
    e2 = G.measure(c["emu", 2], c["ref"], c["den"])
    assert 0 < e3 < G.gamma_rows(F32, G.SHAPES[shape][2])
    assert e3 < e2 < 2.0 ** -16


def test_late_inputs_are_late():
    """Couplings about 1e-6 of the norms, blocks orthogonal inside."""
    c = G.pair_case("late", F64, 32, 2, "full")
    g = c["ref"].sum(1).astype(np.float64)               # (P, 64, 64)
    d = np.sqrt(np.einsum("pii->pi", g))
    rel = np.abs(g) / (d[:, :, None] * d[:, None, :])
    off = rel[:, :32, 32:]
    assert 1e-8 < off.max() < 1e-5
    inside = rel[:, :32, :32] - np.eye(32)
    assert np.abs(inside).max() < 1e-10


def test_zero_blocks_give_zero_denominators():
    c = G.pair_case("zeros", F32, 32, 0, "cross")
    assert (c["den"][2] == 0).all() and (c["den"][0][:, :, -3:] == 0).all()  # block 4; block 5's last columns
    bad = c["emu"].clone()
    bad[2, 0, 3, 4] = 1e-30
    assert _rejected(c, bad)


def test_ints_are_exact_in_every_format():
    for shape in range(len(G.SHAPES)):
        c = G.pair_case("ints", F32, 64, shape, "full")
        ref = c["ref"]
        assert (ref == np.rint(ref)).all() and np.abs(ref).max() < 2 ** 24
        assert (ref.astype(np.float32).astype(np.longdouble) == ref).all()
        assert not _rejected(c, c["emu"])  # any order of fp32 sums gives the same
    q = G.quad_case("ints", 2, 2)
    x = q["At"][:64, :q["m_pad"]]
    p = split_bf16(x, 3)
    assert torch.equal(p[0].float(), x) and not p[1].float().any() and not p[2].float().any()
    for np_ in (3, 2):
        emu = G.emulate_quad(q["At"], q["L"], q["R"], q["m_pad"], q["rows"], np_)
        assert not _rejected(q, emu, np_)


@pytest.mark.parametrize("np_", [3, 2])
def test_parts_split_and_sums_as_claimed(np_):
    c = G.quad_case("parts", 2, 2)  # m_pad 640, chunks of 256 rows
    x = c["At"][:8 * 64, :600]
    k = torch.round(x)
    assert set(k.unique().tolist()) == {1.0, 2.0, 3.0}
    p = [t.double() for t in split_bf16(x, 3)]
    assert torch.equal(p[0], k.double()) and torch.equal(p[1], k.double() * 2.0 ** -9)
    assert torch.equal(p[2], k.double() * 2.0 ** -18)
    lead, rest = G.exact_parts_sums(c["At"], c["L"], c["R"], c["m_pad"], c["rows"], np_)
    assert torch.equal(lead, lead.round()) and 0 < float(lead.max()) <= 5760
    r18 = rest * 2.0 ** 18
    assert torch.equal(r18, r18.round()) and float(rest.max()) < 32
    assert torch.equal(lead.float().double(), lead) and torch.equal(rest.float().double(), rest)
    emu = G.emulate_quad(c["At"], c["L"], c["R"], c["m_pad"], c["rows"], np_)
    bad, fig = G.check(c, emu, np_)
    assert not bad and fig["ulps"] <= 0.5  # one rounding: the final add


# --------------------------------------------------------- planted faults
@pytest.fixture(scope="module")
def full_case():
    return G.pair_case("graded", F32, 32, 2, "full")  # chunks of 256, 256 and 128 rows


@pytest.mark.parametrize("kind", ["graded", "late"])
def test_a_slab_left_out_is_rejected(kind):
    c = G.pair_case(kind, F32, 32, 2, "cross")
    bad = G.emulate_plain(c["At"], c["L"], c["R"], c["m_pad"], c["rows"], skip_slab=(1, 5))
    assert _rejected(c, bad)


def test_swapped_chunks_are_rejected():
    c = G.pair_case("graded", F32, 32, 2, "cross")
    bad = c["emu"][:, [1, 0, 2]].contiguous()       # the sum over the chunks cannot tell
    assert _rejected(c, bad)
    bad = c["emu"][:, [0, 2, 1]].contiguous()       # the short last chunk in another's place
    assert _rejected(c, bad)


def test_a_transposed_slab_is_rejected():
    c = G.pair_case("graded", F32, 32, 2, "cross")
    bad = c["emu"].clone()
    bad[1, 2] = c["emu"][1, 2].t()
    assert _rejected(c, bad)


def test_a_stale_quadrant_is_rejected(full_case):
    W = 32
    for rs, cs in ((slice(0, W), slice(0, W)), (slice(W, None), slice(W, None)),
                   (slice(0, W), slice(W, None)), (slice(W, None), slice(0, W))):
        bad = full_case["emu"].clone()
        bad[2, 1, rs, cs] = float("nan")            # what the GPU tests fill the slabs with
        assert _rejected(full_case, bad)
        bad[2, 1, rs, cs] = full_case["emu"][0, 1, rs, cs]  # or another pair's numbers
        assert _rejected(full_case, bad)


def test_unmirrored_quadrants_are_rejected(full_case):
    W = 32
    bad = full_case["emu"].clone()
    bad[0, 0, W:, :W] = bad[0, 0, :W, W:]           # copied, not transposed
    assert not G.mirrored(bad, W) and _rejected(full_case, bad)
    bad = full_case["emu"].clone()
    bad[0, 0, W, 3] = torch.nextafter(bad[0, 0, W, 3], torch.tensor(float("inf")))  # one bit
    assert _rejected(full_case, bad)


def test_exchanged_quad_slabs_are_rejected():
    c = G.quad_case("graded", 2, 0)
    P = len(c["pairs"])
    for i, j in ((P + 0, P + 1), (P + 2, P + 3), (0, 1), (P + 1, P + 4)):
        bad = c["emu", 3].clone()
        bad[[i, j]] = bad[[j, i]]
        assert _rejected(c, bad, 3)


@pytest.mark.parametrize("np_", [3, 2])
def test_dropped_product_classes(np_):
    """Every product class left out of the quad emulation: the 'parts' check
    rejects it by at least 16 ulp; the 'graded' measure is printed (see the
    module docstring)."""
    p = G.quad_case("parts", 2, 0)
    g = G.quad_case("graded", 2, 0)
    e_ref = G.measure(g["emu", np_], g["ref"], g["den"])
    for d in G.kept_products(np_):
        bad, fig = G.check(p, G.emulate_quad(p["At"], p["L"], p["R"], p["m_pad"], p["rows"], np_,
                                             drop=d), np_)
        assert bad and fig["ulps"] >= 16, (d, fig)
        e = G.measure(G.emulate_quad(g["At"], g["L"], g["R"], g["m_pad"], g["rows"], np_, drop=d),
                      g["ref"], g["den"])
        print(f"GRAM_DROP np{np_} {d} parts {fig['ulps']:.1f} ulp, graded {e / e_ref:.1f} x e_ref")
        assert e > e_ref
        if sum(d) < 2:
            assert e > 10 * RATIO_MAX * e_ref


def test_a_row_read_at_m_pad_is_rejected():
    for kind in ("graded", "ints"):
        c = G.pair_case(kind, F32, 32, 0, "cross")
        bad = G.emulate_plain(c["At"], c["L"], c["R"], c["m_pad"], c["rows"], over_read=True)
        assert torch.isnan(bad).all() and _rejected(c, bad)


def test_a_read_of_the_unnamed_block_is_rejected():
    c = G.pair_case("graded", F32, 32, 0, "cross")
    L = c["L"].clone()
    L[1] = torch.arange(32) + 6 * 32
    assert _rejected(c, G.emulate_plain(c["At"], L, c["R"], c["m_pad"], c["rows"]))
