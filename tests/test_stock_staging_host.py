"""Host: the index arithmetic of the stock networks' first-layer staging (csrc/mlp.hip `net_put_fixed`).  Word j of the
flat 64 x K0 matrix goes to row j // K0 of the padded tile, and the kernel forms that quotient as
`(int)((j + 0.5f) * rcp(K0))` with the hardware's approximate reciprocal (one ulp).  Restated here in float32 with the
reciprocal moved by up to two ulps either way, for every K0 the fixed-shape path admits and every word a tile can hold:
the truncation must be the exact quotient.  Also the slot rule: slot u of a THREADS-wide fetch is issued iff the matrix
has a word at or beyond u * THREADS, and the issued slots cover every word exactly once."""
import numpy as np
import pytest


@pytest.mark.parametrize('ulps', [-2, -1, 0, 1, 2])
def test_reciprocal_quotient_is_the_integer_quotient(ulps):
    j = np.arange(4096, dtype=np.int64)
    for K0 in range(1, 65):
        inv = np.float32(1.0) / np.float32(K0)
        for _ in range(abs(ulps)):
            inv = np.nextafter(inv, np.float32(np.inf if ulps > 0 else -np.inf), dtype=np.float32)
        live = j < 64 * K0
        row = ((j.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)       # float32 product, truncated
        assert np.array_equal(row[live], (j // K0)[live]), K0
        col = j - row * K0
        assert ((col[live] >= 0) & (col[live] < K0)).all(), K0


@pytest.mark.parametrize('threads', [256, 512, 1024])
def test_issued_slots_cover_every_word_once(threads):
    for K0 in range(1, 65):
        words = 64 * K0
        slots = [u for u in range(4096 // threads) if u == 0 or u * threads < words]
        seen = np.zeros(words, dtype=np.int64)
        for u in slots:
            jj = u * threads + np.arange(threads)
            np.add.at(seen, jj[jj < words], 1)
        assert (seen == 1).all(), (threads, K0)
        assert len(slots) == max(1, -(-words // threads)), (threads, K0)
