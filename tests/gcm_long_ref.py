"""The tests' own restatement of the segmented GHASH plans of DESIGN.md 5.16, on top of tests/gcm_ref.py's byte-wise
"times x": a frame's segments, the inner rows and their chunks, and the final rows.  Shared by
tests/test_aes_gcm_long.py (CPU) and tests/test_gpu_gcm_long.py (numpy u64 sums)."""
import numpy as np

from tests import gcm_ref as R


def n_segments(m: int, seg: int) -> int:
    return -(-m // seg)


def segment_blocks(xs, seg, c):
    """X_(c,1) .. X_(c,kc): the hashed blocks of exponents seg c + 1 .. min(seg c + seg, m), exponent e being X_(m+1-e)."""
    m = len(xs)
    return [xs[m - e] for e in range(seg * c + 1, min(seg * c + seg, m) + 1)]


def segment_rows(xs, seg, c, n_rows):
    """rows[r] = the table bits 128 (k - 1) + i with coefficient r of X_(c,k) x^i set, ascending (k, i)."""
    rows = [[] for _ in range(n_rows)]
    for k, col in enumerate(segment_blocks(xs, seg, c), start=1):
        for i in range(128):
            for r in np.flatnonzero(R.coefs(col)[:n_rows]):
                rows[r].append(128 * (k - 1) + i)
            col = R.times_x(col)
    return rows


def inner_chunks(row):
    """Greedy chunks of 64; a row without a source is one empty chunk."""
    return [row[at:at + 64] for at in range(0, len(row), 64)] or [[]]


def long_plan(aad, c, tag_len, seg, n_frames=1, first_product=0):
    """(inner, final): inner[s - 1] the 128 rows of S_s, final the rows r < 8 tag_len over the source array [the
    table's first min(seg, m) blocks, E(J0) of n_frames frames, the products], without the E(J0) bit; the frame's
    products start at product first_product of the call."""
    xs = R.hashed_blocks(aad, c)
    m = len(xs)
    tb = min(seg, m)
    inner = [segment_rows(xs, seg, s, 128) for s in range(1, n_segments(m, seg))]
    final = segment_rows(xs, seg, 0, 8 * tag_len)
    for r, row in enumerate(final):
        row += [128 * (tb + n_frames + first_product + s - 1) + r for s in range(1, n_segments(m, seg))]
    return inner, final
