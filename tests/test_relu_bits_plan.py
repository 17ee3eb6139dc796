"""CPU: the one-bit ReLU image contract between the forward NT launch that writes it and the dgrad launch that reads it ("the bit
image contract"). A forward writes the bit words of its WHOLE tiles, a dgrad reads the bit words of ITS whole tiles; a tile read and never
written is whatever the buffer held before - plausible, wrong gradients and no error. toad_relu_bits_plan reports both sets from the code
that decides the launches (csrc/gemm_f32.hip nt_route / nt_bits_tile_map, csrc/step.hip nt_row_chunks / step_dgrad1_reads_bits), so

    reads(M, N, K_b, reader flags)  is a subset of  writes(M, N, K_f, forward)

is checked here for every shape class, for the row chunks of the per-op wrappers (ops._row_chunks) and for those of the whole-slide calls
(nt_rows), without a GPU. tests/test_gpu_relu_bits.py runs the same pairs on the device over poisoned buffers."""
import numpy as np
import pytest

from toad_amd import _lib, ops

READER, ADDEND, POOL, POOL_BATCHED, A16, APT, SELF_MEASURE, ROWS, STEP_L1 = 1, 2, 4, 8, 16, 32, 64, 128, 256
OK, EINVAL, ESHAPE = 0, -1, -2
CHUNK_ROWS = 4092 * 256                                  # csrc/step.hip kChunkRows
NKS = (1, 2, 3, 4, 16, 24, 32)                           # reduction depths in 32-deep stages
WIDTHS = (4, 256, 260, 384, 512, 768, 1024)
READER_FLAGS = (READER, READER | ADDEND, READER | POOL, READER | POOL_BATCHED)       # every reader the launcher accepts
WRITER_FLAGS = (0, SELF_MEASURE)                         # the plain forward: with the abs-max array of its input, or measuring it itself


def _tiles(m, n):
    return (m + 255) // 256, (n + 255) // 256


def plan(m, n, k, flags, out=None):
    """-> (rc, uint8 map [row tiles, column tiles])"""
    tm, tn = _tiles(m, n)
    buf = np.empty(tm * tn, np.uint8) if out is None else out[:tm * tn]
    rc = _lib.load().toad_relu_bits_plan(m, n, k, flags, buf.ctypes.data)
    return rc, buf.reshape(tm, tn)


def test_query_validates_its_arguments_and_matches_the_documented_cases():
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    assert lib.toad_relu_bits_plan(300, 512, 1024, 0, None) == EINVAL
    assert lib.toad_relu_bits_plan(300, 512, 1024, 1 << 12, buf.ctypes.data) == EINVAL          # unknown flag
    assert lib.toad_relu_bits_plan(300, 512, 1024, A16 | APT, buf.ctypes.data) == EINVAL
    for m, n, k in ((0, 512, 1024), (300, 512, 1000), (300, 510, 1024), (1 << 20, 512, 1024)):   # what toad_linear_h2_ok refuses
        assert not lib.toad_linear_h2_ok(m, n, k)
        assert lib.toad_relu_bits_plan(m, n, k, 0, buf.ctypes.data) == ESHAPE, (m, n, k)
    assert b"toad_linear_h2_ok" in lib.toad_last_error()
    # combinations the launcher refuses: a mask / addend on an fp16 or prepared operand, both addends at once
    for fl in (READER | A16, READER | APT, ADDEND | APT, READER | ADDEND | POOL, SELF_MEASURE | READER, SELF_MEASURE | ADDEND):
        assert lib.toad_relu_bits_plan(3000, 512, 512, fl, buf.ctypes.data) == EINVAL, fl
    # a 256-patch bag: two tiles on two XCDs, sixteen one-stage slices each -> no whole tile, nothing written, nothing read
    for fl in (0, READER):
        rc, mp = plan(256, 512, 512, fl)
        assert rc == OK and not mp.any()
    # 10,000 rows x 512: the half-height case (csrc/gemm_f32.hip nt_half_tiles) - forward and dgrad touch every tile; an addend buffer keeps
    # the dgrad on 256-row tiles, where it reads whole tiles only
    for fl in (0, SELF_MEASURE, READER, READER | POOL, READER | POOL_BATCHED):
        rc, mp = plan(10000, 512, 768, fl)
        assert rc == OK and (mp == 2).all(), fl
    rc, mp = plan(10000, 512, 768, READER | ADDEND)
    assert rc == OK and (mp <= 1).all()
    # 100,000 rows x 512 (the benchmark's bag): 782 tiles = 3 full rounds of 256 workgroups + 14 remainder tiles, which are split
    rc, mp = plan(100000, 512, 1024, 0)
    assert rc == OK and int(mp.sum()) == 768 and mp.size == 782


def _sweep_ms():
    for t in range(1, 4201):                              # every row-tile count past kChunkRows / 256 = 4,092
        r0 = (t - 1) * 256
        yield from (r0 + 1, r0 + 128, r0 + 129, r0 + 256)  # the tile's first row, its 128th and 129th (the half-tile rule counts 128-row tiles), its last


@pytest.mark.parametrize("n", WIDTHS)
def test_single_launch_reads_are_a_subset_of_writes(n):
    """Every (M, N), every forward depth K_f against every reader depth K_b and every reader the launcher accepts: what one dgrad launch reads
    of the image, one forward launch of the same (M, N) wrote. Shapes toad_linear_h2_ok refuses must come back as TOAD_ESHAPE."""
    lib = _lib.load()
    fn = lib.toad_relu_bits_plan
    tn = (n + 255) // 256
    cap = 4200 * tn
    wbuf = np.empty((len(NKS) * len(WRITER_FLAGS), cap), np.uint8)
    rbuf = np.empty((len(NKS) * len(READER_FLAGS), cap), np.uint8)
    wptr = [wbuf[i].ctypes.data for i in range(wbuf.shape[0])]
    rptr = [rbuf[i].ctypes.data for i in range(rbuf.shape[0])]
    checked = refused = halves = 0
    for m in _sweep_ms():
        nt = ((m + 255) // 256) * tn
        wrows, rrows = [], []
        for i, nk in enumerate(NKS):
            k = 32 * nk
            ok = bool(lib.toad_linear_h2_ok(m, n, k))
            for j, fl in enumerate(WRITER_FLAGS):
                rc = fn(m, n, k, fl, wptr[i * len(WRITER_FLAGS) + j])
                assert rc == (OK if ok else ESHAPE), (m, n, k, fl, rc)
                if ok:
                    wrows.append(i * len(WRITER_FLAGS) + j)
            for j, fl in enumerate(READER_FLAGS):
                rc = fn(m, n, k, fl, rptr[i * len(READER_FLAGS) + j])
                if not ok:
                    assert rc == ESHAPE, (m, n, k, fl, rc)
                    continue
                # the one reader the launcher turns down: the batched pooled addend exists on the bit image only, and a one-stage reduction
                # that may not use the image (its whole tiles are not the forward's) has no kernel for it - an error, never a wrong mask
                if rc == EINVAL and fl == READER | POOL_BATCHED and nk == 1:
                    continue
                assert rc == OK, (m, n, k, fl, rc)
                rrows.append(i * len(READER_FLAGS) + j)
            refused += not ok
        if not wrows:
            continue
        w = wbuf[wrows, :nt]
        written = w.min(axis=0)                             # tiles EVERY forward of this (M, N) wrote, whatever its depth
        r = rbuf[rrows, :nt]
        bad = (r != 0) & (written == 0)
        assert not bad.any(), f"M={m} N={n}: reader rows {np.unique(np.nonzero(bad)[0])} of {rrows} read tiles {np.nonzero(bad)[1][:8]} that a forward left unwritten"
        # half-height tiles are never split: a launch on that path touches every tile, and a dgrad on it reads every tile
        for maps in (w, r):
            on_half = (maps == 2).any(axis=1)
            assert ((maps[on_half] == 2).all(axis=1)).all(), (m, n)
            halves += int(on_half.sum())
        if (r == 2).any():
            assert (w != 0).all(), (m, n)
        checked += 1
    assert checked == 4200 * 4 and halves > 0                  # the sweep ran: every count up to the 32-bit limit of the deepest operand, both tile heights
    assert refused > 0                                      # ... and went past that limit (4,097 tiles and more at K = 1024)


# ---- the per-op wrappers: row chunks decided in Python (ops._row_chunks) ----------------------------------------------------------------

BIG_M = (1_047_552, 1_047_553, 1_048_576, 1_049_600, 1_398_101, 1_398_102, 2_097_151, 2_097_152, 4_200_000)


def _per_op_forward_image(m, n, k):
    """What ops.linear_act_fwd(x [m,k], w [n,k], want_bits=True) leaves in its image: None when it returns no image, else the tile map, each
    chunk's launch writing the 256-row blocks of its rows."""
    chunks = ops._row_chunks(m, k * 4)
    if not ops._bits_chunks_ok(m, k * 4):
        return None
    tm, tn = _tiles(m, n)
    img = np.zeros((tm, tn), np.uint8)
    for r0, r1 in chunks:
        assert r0 % 256 == 0
        rc, mp = plan(r1 - r0, n, k, SELF_MEASURE)            # (x_amax = None, as functional.trunk_scores calls layer 1; 0 gives the same map)
        assert rc == OK, (m, n, k, r0, r1)
        rc0, mp0 = plan(r1 - r0, n, k, 0)
        assert rc0 == OK and np.array_equal(mp, mp0)
        img[r0 // 256:(r1 + 255) // 256] = mp
    return img


def _per_op_dgrad_reads(m, n, kb, flags, have_image):
    """What ops.linear_dgrad(dy [m,kb], wt [n,kb], relu_src [m,n], relu_bits=image) reads of the image, chunk by chunk."""
    tm, tn = _tiles(m, n)
    reads = np.zeros((tm, tn), np.uint8)
    if not have_image or not ops._bits_chunks_ok(m, kb * 4):
        return reads
    for r0, r1 in ops._row_chunks(m, kb * 4):
        assert r0 % 256 == 0
        rc, mp = plan(r1 - r0, n, kb, flags)
        assert rc == OK, (m, n, kb, r0, r1)
        reads[r0 // 256:(r1 + 255) // 256] = mp
    return reads


@pytest.mark.parametrize("m", BIG_M)
@pytest.mark.parametrize("size_arg", ["big", "small"])
def test_per_op_row_chunks_keep_reads_inside_writes(size_arg, m):
    """functional.mil_forward / mil_backward on a bag of m patches: layer 1 (1024 -> 512) is read back by the 512-deep dgrad of layer 2, layer 2
    (512 -> 512) by the 2D-deep dgrad of the stacked attention Linear with the pooling addend. The forwards chunk their INPUT rows, the dgrads
    their dY rows - operands of different widths."""
    d2 = 2 * (384 if size_arg == "big" else 256)
    for (kf, n, kb, fl) in ((1024, 512, 512, READER), (512, 512, d2, READER | POOL), (512, 512, d2, READER | ADDEND)):
        img = _per_op_forward_image(m, n, kf)
        reads = _per_op_dgrad_reads(m, n, kb, fl, img is not None)
        if img is None:
            assert not reads.any()
            continue
        bad = np.nonzero((reads != 0) & (img == 0))
        assert bad[0].size == 0, (f"m={m} {kf}->{n}, dgrad depth {kb}: {bad[0].size} tiles read and never written, first (row tile, column tile) "
                                  f"{(int(bad[0][0]), int(bad[1][0]))}; forward chunks {ops._row_chunks(m, kf * 4)}, dgrad chunks {ops._row_chunks(m, kb * 4)}")


def test_per_op_chunks_are_the_whole_slide_chunks():
    """Operands of at most 1024 floats per row are cut by rows alone, at the places csrc/step.hip nt_rows cuts them; wider rows take shorter
    chunks and neither produce nor consume an image."""
    for m in (1, 4092 * 256, 4092 * 256 + 1, 1_049_600, 4_200_000):
        want = [(0, m)] if m <= CHUNK_ROWS else [(r0, min(m, r0 + CHUNK_ROWS)) for r0 in range(0, m, CHUNK_ROWS)]
        for row_bytes in (4, 128, 2048, 3072, 4096):
            assert ops._row_chunks(m, row_bytes) == want and ops._bits_chunks_ok(m, row_bytes)
            assert all((r1 - r0) * row_bytes < (1 << 32) for r0, r1 in want)
    wide = ops._row_chunks(600_000, 8192)
    assert len(wide) == 2 and all((r1 - r0) * 8192 < (1 << 32) and r0 % 256 == 0 for r0, r1 in wide) and not ops._bits_chunks_ok(600_000, 8192)
    assert ops._row_chunks(500_000, 8192) == [(0, 500_000)] and ops._bits_chunks_ok(500_000, 8192)


# ---- the whole-slide calls: row chunks decided in C (nt_rows) ----------------------------------------------------------------------------

@pytest.mark.parametrize("m", (64, 300, 2000, 4097, 10000, 16500, 40000) + BIG_M)
def test_whole_slide_row_chunks_keep_reads_inside_writes(m):
    """TOAD_BITS_ROWS composes the query over the launches nt_rows makes. Layer 2 (512 -> 512, dgrad depth 512 / 768 with the pooling addend,
    plain and batched) for fp32 operands; layer 1 through TOAD_BITS_STEP_L1 for fp32, fp16 and prepared bags, whose first Linear runs on 256-row
    tiles while the dgrad behind it may run on half-height tiles (step_dgrad1_reads_bits)."""
    tm, tn = _tiles(m, 512)
    rc, w2 = plan(m, 512, 512, ROWS)
    assert rc == OK
    if m > CHUNK_ROWS:                                          # the composition really is per chunk: the last chunk's map is that of a launch of its rows
        last = m - (m - 1) // CHUNK_ROWS * CHUNK_ROWS
        rc, tail = plan(last, 512, 512, 0)
        assert rc == OK and np.array_equal(w2[(m - 1) // CHUNK_ROWS * 4092:], tail)
    for kb in (512, 768):
        for fl in (READER | POOL, READER | POOL_BATCHED, READER, READER | ADDEND):
            rc, r = plan(m, 512, kb, fl | ROWS)
            assert rc == OK, (m, kb, fl)
            assert not ((r != 0) & (w2 == 0)).any(), (m, kb, fl)
    for bag in (0, A16, APT):
        rcw, w1 = plan(m, 512, 1024, STEP_L1 | bag)
        rcr, r1 = plan(m, 512, 512, STEP_L1 | READER | bag)
        if bag and (m > CHUNK_ROWS or not _lib.load().toad_linear_h2_ok(m, 512, 1024)):
            assert rcw == ESHAPE and rcr == ESHAPE              # fp16 / prepared bags are one launch: no row chunks
            continue
        assert rcw == OK and rcr == OK, (m, bag)
        assert not ((r1 != 0) & (w1 == 0)).any(), (m, bag)
        if bag:                                                 # 256-row tiles only, and where the dgrad would read every tile it gets no image
            assert (w1 <= 1).all()
            rc, plain_reader = plan(m, 512, 512, READER)
            assert rc == OK
            assert not r1.any() if (plain_reader == 2).any() else np.array_equal(r1, plain_reader)
    assert plan(m, 512, 512, STEP_L1)[0] == ESHAPE and plan(m, 256, 1024, STEP_L1)[0] == ESHAPE     # STEP_L1 is that one pair of launches
