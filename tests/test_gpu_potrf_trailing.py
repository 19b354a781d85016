"""-m gpu: the two trailing-update roles of the fused Cholesky that have a knob of their own.

Tile loop (IPM_STILE_LOOP=1 / 2): the lazy-C 128 x 128 trailing tiles with both operands staged
through LDS, or with the X fragments loaded straight into the MFMA operand registers.  Every
accumulator receives the same products and the same C block in the same order, so the factors
are bitwise equal.

Ragged rows (IPM_RAG=0 / 1): the 1-8 trailing rows past a multiple of 128 as a row of 128-tiles,
or by the ragged-row workgroups (K split over the four waves, partial sums added in wave order):
another summation order, so equal to fp64 rounding only, but the same bits on every call.

Which kernel each launch runs was confirmed with IPM_PLAN_DEBUG=1 (one line per launch: kernel
0 / 1 = lazy-C K = 256 / K = 512 tiles on loop 1, 5 / 6 = the same on loop 2, and the ragged-row
workgroup count with its K):
  n = 1024:                  blocks 1, 2 run kernel 0 / 5 (10 and 3 tiles, K = 256)
  n = 1536, IPM_PAIR_MIN=512: block 2 runs kernel 1 / 6 (21 tiles, K = 512), blocks 3, 4 kernel 0 / 5
  n = 1030, IPM_RAG=1:       blocks 1, 2 run kernel 0 / 5 with 5 and 3 ragged-row workgroups
  n = 1537, IPM_PAIR_MIN=512, IPM_RAG=1: block 2 has 7 ragged-row workgroups with K = 512
"""
import pytest

pytestmark = pytest.mark.gpu


def _spd(n, seed):
    """the matrices of test_potrf_ragged_rows"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    M = torch.rand((n + 5, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
    return M.T @ M + n * torch.eye(n, dtype=torch.float64, device="cuda")


def _factor(A, n, ncols, lda=None):
    """factor a copy of A (leading dimension lda); the whole lower triangle of the buffer"""
    import torch
    from gpu_util import potrf
    lda = lda or n
    H = torch.zeros(n, lda, dtype=torch.float64, device="cuda")
    H[:, :n] = A   # symmetric: the column-major buffer is A itself
    rc, info = potrf(H, n, lda, ncols=ncols)
    assert rc == 0 and info == 0
    return torch.tril(H[:, :n].T)


def _check_against_torch(A, L, n, ncols):
    import torch
    L11 = torch.linalg.cholesky(A[:ncols, :ncols])
    e11 = ((L[:ncols, :ncols] - L11).abs().max() / L11.abs().max()).item()
    print(f"vs torch: L11 {e11:.3e}")
    assert e11 < 1e-10
    if ncols < n:
        L21 = torch.linalg.solve_triangular(L11, A[ncols:, :ncols].T, upper=False).T
        e21 = ((L[ncols:, :ncols] - L21).abs().max() / L21.abs().max()).item()
        print(f"vs torch: L21 {e21:.3e}")
        assert e21 < 1e-10


@pytest.mark.parametrize("n,env", [
    (1024, {}),                                        # K = 256 lazy-C tiles (LAZY 1)
    (1536, {"IPM_PAIR_MIN": "512"}),                   # a pair launch: K = 512 tiles (LAZY 2)
    (1030, {}),                                        # ragged edge as tiles: the general loop
    (1030, {"IPM_RAG": "1"}),                          # ragged edge split off: lazy-C tiles beside it
])
def test_trailing_tile_loops_are_bitwise_equal(n, env, monkeypatch):
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A = _spd(n, n)
    out = {}
    for loop in ("1", "2"):
        monkeypatch.setenv("IPM_STILE_LOOP", loop)
        out[loop] = _factor(A, n, n)
    assert torch.equal(out["2"], out["1"])
    _check_against_torch(A, out["2"], n, n)


@pytest.mark.parametrize("n,ncols,lda,env", [
    (641, 640, None, {}),                              # one right-hand-side row, not factored
    (648, 648, None, {}),                              # eight ragged rows
    (1030, 1030, None, {}),                            # the existing mixed case (6 rows)
    (1537, 1536, None, {"IPM_PAIR_MIN": "512"}),       # a pair launch: rag_K = 512
    (1030, 1030, 1031, {}),                            # an odd leading dimension
    (431, 301, 432, {}),                               # an odd origin: 8-byte loads throughout
])
def test_ragged_row_role(n, ncols, lda, env, monkeypatch):
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A = _spd(n, n)
    out = {}
    for mode in ("0", "1", "1"):
        monkeypatch.setenv("IPM_RAG", mode)
        L = _factor(A, n, ncols, lda)
        if mode == "1" and mode in out:
            assert torch.equal(L, out[mode]), "a second call differs"
        out[mode] = L
    # (the whole triangle: with ncols < n the ragged rows also lie in the partly updated columns
    # right of the factored ones -- visible where the buffer is factored in place, a leading
    # dimension of whole 128-byte lines as in the odd-origin case; any other layout is factored in
    # an aligned copy of which only the factored columns come back)
    scale = out["0"][:, :ncols].abs().max()
    d = ((out["1"] - out["0"]).abs().max() / scale).item()
    print(f"IPM_RAG=1 vs 0: {d:.3e}")
    assert d < 1e-12
    _check_against_torch(A, out["1"], n, ncols)
