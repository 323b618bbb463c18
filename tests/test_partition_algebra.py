"""CPU: the partition (reduced-interface) algebra of cmc_fluid_solver_amd/partition.py -- what csrc/kernels_part.hip
executes inside a workgroup / a wave and what the cross-slab X solve executes across ranks -- against the sequential
Thomas solve of the oracle (pinned bit for bit to the reference's Common/Algorithms.h, tests/test_oracle_pins.py).
Algebraically exact: fp64 agrees to round-off, fp32 to a few ulp of the solution norm."""
import numpy as np
import pytest

from cmc_fluid_solver_amd import partition as pt


def _system(n, nlines, dtype, seed, nrhs=4):
    """rows shaped like the solver's: weakly dominant interior rows b = 3/dt + 2 vis, a/c = -vis -+ q, BC rows at the ends"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-130, 130, (n, nlines))
    a = (-q - 325.0).astype(dtype); c = (q - 325.0).astype(dtype); b = np.full((n, nlines), 680.0, dtype)
    a[0] = 0; b[0] = 1; c[0] = 0            # NOSLIP start row
    a[-1] = -1; b[-1] = 2; c[-1] = 0        # FREE end row
    d = rng.uniform(-5, 5, (n, nrhs, nlines)).astype(dtype)
    return a, b, c, d


def _thomas_ref(a, b, c, d):
    from oracle import oracle as O
    n, nrhs, nl = d.shape
    out = np.empty((n, nrhs, nl), np.float64)
    for l in range(nl):
        for r in range(nrhs):
            out[:, r, l] = O.tridiag(a[:, l].astype(np.float64), b[:, l].astype(np.float64), c[:, l].astype(np.float64),
                                     np.ascontiguousarray(d[:, r, l], np.float64))
    return out


CASES = [(256, list(range(0, 257, 16))),            # X / Y sweeps: 16 chunks of 16 cells per line
         (256, list(range(0, 257, 4))),             # Z sweep: 64 lanes x 4 cells
         (128, list(range(0, 129, 4))),
         (37, [0, 5, 6, 20, 37]),                   # ragged chunks, one of a single cell
         (256, [0, 32, 64, 96, 128, 160, 192, 224, 256])]     # 8 x-slabs of 32 planes


@pytest.mark.parametrize("reduced", ["thomas", "pcr"])
@pytest.mark.parametrize("n,bounds", CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_partition_solve_equals_thomas(built, dtype, n, bounds, reduced):
    a, b, c, d = _system(n, 12, dtype, seed=n + len(bounds))
    x = pt.solve(a, b, c, d, bounds, reduced)
    ref = _thomas_ref(a, b, c, d)
    err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    assert err <= (5e-15 if dtype == np.float64 else 5e-7), err
    # the solution satisfies the rows (independent of any reference solve)
    x64 = x.astype(np.float64)
    res = b[:, None].astype(np.float64) * x64 - d
    res[1:] += a[1:, None] * x64[:-1]
    res[:-1] += c[:-1, None] * x64[1:]
    assert np.abs(res).max() <= (1e-9 if dtype == np.float64 else 2e-2) * 1.0


def test_identity_rows_decouple_segments():
    """SKIP rows (identity, d = 0) between two segments of a line: each segment's solution is its own Thomas solve."""
    rng = np.random.default_rng(3)
    n, nl = 64, 5
    a, b, c, d = _system(n, nl, np.float64, 9, nrhs=1)
    for s in (20, 21, 22):
        a[s] = 0; b[s] = 1; c[s] = 0; d[s] = 0
    a[23] = 0; c[19] = 0                    # START of the second segment, END of the first
    x = pt.solve(a, b, c, d, list(range(0, 65, 8)))
    ref = _thomas_ref(a, b, c, d)
    assert np.abs(x - ref).max() <= 1e-12
    assert np.abs(x[20:23]).max() == 0


# ---- two segments per line, every end row FREE or NOSLIP, at every chunk offset: the per-line criterion ---------------------
# What tests/test_gpu_bc_matrix.py holds the kernels to, on the model of their chunkings: per right-hand side, S = max |x64|,
# e(K) = max over lines of max |K - x64| / S, and e(partition fp32) <= F e(sequential fp32) + 2^-23 with F = 2.  The model uses
# plain reciprocals, coarser than the kernels' corrected quotients, so F rests on it and not on the kernels.
F_LINE, FLOOR = 2.0, 2.0 ** -23
COEFS = [(5.6, 41.1, 6.0), (312.0, 655.0, 44.0), (1250.0, 2530.0, 90.0)]   # (vis, b, max |q|): the solver's rows at h = 0.03, 0.004 and 0.002
CHUNKINGS = [(16, "thomas"), (4, "pcr")]                # X / Y sweeps; Z sweep
# the line lengths of tests/launch_shape_cases.py too: 260, 388, 512 are 32 chunks of 16 cells (the sequential interface solve over 64
# unknowns) and 128 lanes of 4 (cyclic reduction over 128 unknowns); 72 / 130 and 68 / 132 leave the last chunk and the last lanes
# partly empty; 8-cell chunks with the sequential interface solve are the thin-slab instance (24 and 32 planes)
MORE_LINES = [(72, 16, "thomas"), (130, 16, "thomas"), (68, 4, "pcr"), (132, 4, "pcr"), (24, 8, "thomas"), (32, 8, "thomas")]


def _two_segment_system(n, chunk, coef, dtype, seed, nrhs=4):
    """One line per (kinds of the four end rows) x (offset of the inner END in a chunk) x (gap): segment [0, e], identity rows,
    segment [s, n - 1].  FREE START is b 2, c -1; FREE END is a -1, b 2; NOSLIP is the identity row.  gap 1: END and START on
    adjacent cells (s = e + 1, the END on offset r, the START on r + 1); gap chunk + 1 moves the START to every offset too."""
    vis, bb, qmax = coef
    rng = np.random.default_rng(seed)
    lines = []
    base = 16 if n >= 48 else 8                            # the chunk that the inner rows scan
    for kinds in range(16):
        for r in range(chunk):
            for gap in (1, 3, chunk + 1):
                e = base + r
                s = e + gap
                if s + 2 < n:
                    lines.append((kinds, e, s))
    nl = len(lines)
    q = rng.uniform(-qmax, qmax, (n, nl))
    a = (-q - vis).astype(dtype); c = (q - vis).astype(dtype); b = np.full((n, nl), bb, dtype)
    d = rng.uniform(-5, 5, (n, nrhs, nl)).astype(dtype)
    for l, (kinds, e, s) in enumerate(lines):
        a[e + 1:s, l] = 0; b[e + 1:s, l] = 1; c[e + 1:s, l] = 0; d[e + 1:s, :, l] = 0           # identity rows between the segments
        for bit, cell, start in ((1, 0, True), (2, e, False), (4, s, True), (8, n - 1, False)):
            free = bool(kinds & bit)
            a[cell, l], b[cell, l], c[cell, l] = (0, 2, -1) if free and start else ((-1, 2, 0) if free else (0, 1, 0))
            if free:
                d[cell, :, l] = rng.uniform(-0.01, 0.01, nrhs)
    return a, b, c, d


def _thomas_numpy(a, b, c, d):
    """The sequential recurrence (Common/Algorithms.h:21-38) in the arrays' own precision, every line at once."""
    n = a.shape[0]
    cp = np.empty_like(c); dp = np.empty_like(d)
    cp[0] = c[0] / b[0]; dp[0] = d[0] / b[0][None]
    for i in range(1, n):
        m = b[i] - a[i] * cp[i - 1]
        cp[i] = c[i] / m
        dp[i] = (d[i] - a[i][None] * dp[i - 1]) / m[None]
    x = np.empty_like(d)
    x[n - 1] = dp[n - 1]
    for i in range(n - 2, -1, -1):
        x[i] = dp[i] - cp[i][None] * x[i + 1]
    return x


def _line_error(K, x64):
    S = np.abs(x64).max(axis=(0, 2))                         # per right-hand side
    return (np.abs(K.astype(np.float64) - x64).max(axis=0) / S[:, None]).max(axis=1)      # worst line, per right-hand side


@pytest.mark.parametrize("chunk,reduced", CHUNKINGS)
@pytest.mark.parametrize("coef", COEFS, ids=["h0.03", "h0.004", "h0.002"])
@pytest.mark.parametrize("n", [44, 48, 64, 128, 256, 260, 388, 512])
def test_two_segments_every_end_row_kind_per_line(n, coef, chunk, reduced):
    two_segments_per_line(n, coef, chunk, reduced)


@pytest.mark.parametrize("coef", COEFS, ids=["h0.03", "h0.004", "h0.002"])
@pytest.mark.parametrize("n,chunk,reduced", MORE_LINES)
def test_two_segments_partly_filled_and_thin_slab_chunkings_per_line(n, chunk, reduced, coef):
    two_segments_per_line(n, coef, chunk, reduced)


def two_segments_per_line(n, coef, chunk, reduced):
    a, b, c, d = _two_segment_system(n, chunk, coef, np.float32, seed=n + chunk)
    a64, b64, c64, d64 = (v.astype(np.float64) for v in (a, b, c, d))
    bounds = list(range(0, n, chunk)) + [n]
    x64 = _thomas_numpy(a64, b64, c64, d64)
    # fp64: the partition solve is the same solution
    p64 = pt.solve(a64, b64, c64, d64, bounds, reduced)
    assert np.linalg.norm(p64 - x64) / np.linalg.norm(x64) <= 5e-15
    e_part = _line_error(pt.solve(a, b, c, d, bounds, reduced), x64)
    e_seq = _line_error(_thomas_numpy(a, b, c, d), x64)
    print("n %d, %s chunks of %d, vis %g: e(partition) %s, e(sequential) %s, ratio %s" % (
        n, reduced, chunk, coef[0], ["%.2e" % v for v in e_part], ["%.2e" % v for v in e_seq], ["%.2f" % (p / s) for p, s in zip(e_part, e_seq)]))
    assert (e_seq > 0).all()
    assert (e_part <= F_LINE * e_seq + FLOOR).all()
