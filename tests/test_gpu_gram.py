"""The Gram stage of csrc/hip/block.hip alone (block_gram.hpp gram_kernel and
gram_cross_f32_kernel through kernels.gram_cross / gram_full, block_quad.hpp
gram_quad_kernel through kernels.gram_quad), every slab of every row chunk
against a numpy.longdouble product of the same chunk (tests/_gram_ref.py).

Bound: max |C - C_ref| / (|A_L|^T |A_R|) of the kernel at most RATIO_MAX = 4
times that of the CPU emulation in the data precision on the same inputs;
exact zeros where the denominator is zero.  The kinds 'ints' (equal to the
exact product in every instantiation and chunking) and 'parts' (quad Gram:
within one fp32 ulp of the exact sum of the kept products) have exact answers.
Every input holds NaN past m_pad and in a block no pair names, the slabs are
handed over full of NaN (an entry left unwritten shows), every case runs
twice and the two results must be equal bit for bit (no float atomics).
Every case prints "GRAM_RATIO {json}" before it asserts; the figures measured
on an MI355X are in profiles/gram_alone/: kernel / emulation 0.63 .. 1.66 for
the fp32 and fp64 kernels, 1.14 .. 2.00 for the quad Gram on 3 parts, 0.99 ..
1.01 on 2 parts (the dropped products set the error, alike in both); 'ints'
exact everywhere; 'parts' 0.5 ulp on 3 parts, 0 on 2.

  gram_kernel<float,32,CROSS>, <double,32,CROSS>, <double,64,CROSS> (two row
  halves over blockIdx.z), gram_cross_f32_kernel         test_pair_gram cross
  gram_kernel<float,32,FULL>, <float,64,FULL>, <double,32,FULL>,
  gram_kernel<double,64,SPLIT>                            test_pair_gram full
  gram_quad_kernel<0,3>, <0,2>, two quads and one         test_quad_gram
"""
import ctypes as C
import json

import pytest
import torch

import _gram_ref as G

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _bits(x):
    return x.view(torch.int32 if x.dtype == F32 else torch.int64)


def _twice(run, shape, dtype, cuda):
    """run(out) on slabs full of NaN, twice; the first result on the CPU."""
    outs = []
    for _ in range(2):
        out = torch.full(shape, float("nan"), dtype=dtype, device=cuda)
        assert run(out) is out
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two runs differ"
    return outs[0]


def _verdict(tag, case, got, np_=None):
    bad, fig = G.check(case, got, np_)
    print("GRAM_RATIO " + json.dumps({"case": tag, **fig}))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("kind", G.KINDS + ("ints",))
@pytest.mark.parametrize("shape", range(len(G.SHAPES)))
@pytest.mark.parametrize("mode", ["cross", "full"])
@pytest.mark.parametrize("dtype,W", [(F32, 32), (F32, 64), (F64, 32), (F64, 64)])
def test_pair_gram(svdj, cuda, dtype, W, mode, shape, kind):
    """The cross and the full Gram of the pairs (0,5), (3,1), (2,4) of 7
    blocks (block 6: NaN) at m / m_pad / rows per chunk = 100/128/128 (one
    slab per wave, no prefetch), 256/256/256 (one chunk, the prefetch path),
    600/640/256 (three chunks, a short last one) and 384/384/128."""
    K = svdj.ops.kernels
    case = G.pair_case(kind, dtype, W, shape, mode)
    At = case["At"].to(cuda)
    pairs = torch.tensor(case["pairs"], dtype=torch.int32, device=cuda)
    fn = K.gram_full if mode == "full" else K.gram_cross
    got = _twice(lambda out: fn(At, case["m_pad"], pairs, W, case["rows"], out=out),
                 case["ref"].shape, dtype, cuda)
    _verdict(f"{mode}/{str(dtype)[6:]}/W{W}/m_pad{case['m_pad']}x{case['rows']}/{kind}", case, got)


@pytest.mark.parametrize("kind", G.KINDS + ("ints", "parts"))
@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("nquads", [2, 1])
@pytest.mark.parametrize("parts", [3, 2])
def test_quad_gram(svdj, cuda, parts, nquads, shape, kind):
    """The six cross Grams of the quads (a, b, c, d) = (5,0,3,6), (2,7,1,4) of
    9 blocks (block 8: NaN), and of the first alone (P = 2), at m_pad / rows
    128/128 (four slabs: the prologue is the whole pipeline), 256/256 and
    640/256, on 3 and on 2 bf16 parts."""
    K = svdj.ops.kernels
    case = G.quad_case(kind, nquads, shape)
    At = case["At"].to(cuda)
    pairs = torch.tensor(case["pairs"], dtype=torch.int32, device=cuda)
    got = _twice(lambda out: K.gram_quad(At, case["m_pad"], pairs, 64, case["rows"], parts=parts,
                                         out=out), case["ref"].shape, F32, cuda)
    _verdict(f"quad/np{parts}/q{nquads}/m_pad{case['m_pad']}x{case['rows']}/{kind}", case, got,
             parts)


def test_gram_cross_without_out_allocates(svdj, cuda):
    """The call of the older tests: no ``out``, fp32, the slabs allocated."""
    K = svdj.ops.kernels
    case = G.pair_case("ints", F32, 32, 3, "cross")
    pairs = torch.tensor(case["pairs"], dtype=torch.int32)
    got = K.gram_cross(case["At"].to(cuda), case["m_pad"], pairs, 32, case["rows"]).cpu()
    assert not G.check(case, got)[0]


def test_gram_hook_rejects_bad_arguments(svdj, cuda):
    """svdj_gram itself (not the Python wrapper's own checks): an unsupported
    dtype or W, lda < m_pad, rows that are no multiple of SVDJ_ROW_ALIGN, an
    odd lda for fp32 W = 64, a mode that is neither cross nor full.  Nothing is
    launched: the slabs stay as they were."""
    K = svdj.ops.kernels
    lib = svdj.ops.hip_lib()
    At = torch.zeros(4 * 64, 256, dtype=F64, device=cuda)  # room for every call below
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device=cuda)
    out = torch.full((4 * 128 * 128,), 3.0, dtype=F64, device=cuda)

    def call(dtype=0, W=32, mode=K.STEP_CROSS, lda=256, m_pad=128, rows=128):
        rc = lib.svdj_gram(dtype, W, mode, C.c_void_p(At.data_ptr()), lda, m_pad,
                           C.c_void_p(pairs.data_ptr()), 1, rows, C.c_void_p(out.data_ptr()),
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, lib.svdj_hip_last_error().decode()

    assert call(dtype=2)[0] == -3 and call(W=48)[0] == -3 and call(dtype=1, W=16)[0] == -3
    assert call(lda=127)[0] == -2
    assert call(rows=96)[0] == -2 and call(rows=0)[0] == -2 and call(m_pad=100)[0] == -2
    rc, msg = call(W=64, lda=129)
    assert rc == -2 and "multiple of 4" in msg
    assert call(W=64, lda=130, mode=K.STEP_FULL)[0] == -2
    assert call(mode=K.STEP_QUAD)[0] == -2 and call(mode=-1)[0] == -2
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    with pytest.raises(svdj.ops.NativeError):
        K.gram_full(At.float(), 128, pairs, 64, 96)
    with pytest.raises(ValueError):
        K.gram_cross(At.float(), 128, pairs, 32, 128, out=out[:32 * 32].view(1, 1, 32, 32))
