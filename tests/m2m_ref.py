"""Reference for the mask-to-mask fan-out (csrc/mask_prompt.hip m2m_fanout_kernel, `infer_masks(m2m=True)`, `generate(use_m2m=True)`), plain
numpy.

`fanout` restates cvmi_m2m_fanout: every candidate of a pass becomes a pair of the next -- its plane clamped as torch.clamp does (a NaN stays,
-0.0 stays, +-inf become +-c), candidate-major inside its pair, and its pair's prompt rows beside it, each row written NM times.
tests/test_m2m_ref_cpu.py holds it to torch.clamp / repeat_interleave and shows that the comparison of the GPU test rejects the wrong
orders, a missing clamp, a NaN-dropping clamp and tiled tables."""
import numpy as np

MUTANTS = ("point_major", "no_clamp", "nan_to_bound", "tiled_tables")
UPSTREAM_CLAMP = 32.0

# the kernel's loop: at most 64 workgroups of 256 threads per pair, 4 floats per thread and step -> floats of one pair one pass covers
GRID_PASS_FLOATS = 64 * 256 * 4
# (n, NM, P, K); the last row's NM * P = 98316 floats per pair need a second, partial pass of the grid-stride loop at the grid cap
ROWS = ((1, 1, 4, 1), (5, 3, 36, 2), (7, 3, 4096, 4), (2, 3, 32772, 3))
assert ROWS[-1][1] * ROWS[-1][2] > GRID_PASS_FLOATS and (ROWS[-1][1] * ROWS[-1][2]) % GRID_PASS_FLOATS != 0


def clamp(x, c):
    """torch.clamp(x, -c, c) on f32 by comparisons: a NaN fails both and stays."""
    x = np.asarray(x, dtype=np.float32)
    c = np.float32(c)
    out = x.copy()
    out[x < -c] = -c
    out[x > c] = c
    return out


def fanout(low_res, c, coords, labels, pair_image=None, mutant=None):
    """low_res f32 [n, NM, P], coords f32 [n, K, 2], labels i32 [n, K], pair_image i32 [n] or None
    -> (mask f32 [n * NM, P], coords [n * NM, K, 2], labels [n * NM, K], pair_image [n * NM] or None)."""
    low_res = np.asarray(low_res, dtype=np.float32)
    n, NM, P = low_res.shape
    c32 = np.float32(c)
    if mutant == "no_clamp":
        planes = low_res.copy()
    elif mutant == "nan_to_bound":
        planes = np.fmin(np.fmax(low_res, -c32), c32)                       # fminf / fmaxf: a NaN becomes a bound
    else:
        planes = clamp(low_res, c32)
    if mutant == "point_major":
        mask = planes.transpose(1, 0, 2).reshape(n * NM, P)                # row k * n + i
    else:
        mask = planes.reshape(n * NM, P)                                   # row i * NM + k
    if mutant == "tiled_tables":
        rep = lambda a: np.concatenate([a] * NM, 0)                        # rows 0 .. n-1, then again
    else:
        rep = lambda a: np.repeat(a, NM, axis=0)                           # row i at i * NM .. i * NM + NM - 1
    return (np.ascontiguousarray(mask), rep(np.asarray(coords, dtype=np.float32)), rep(np.asarray(labels, dtype=np.int32)),
            None if pair_image is None else rep(np.asarray(pair_image, dtype=np.int32)))


def specials(c):
    """The values the clamp is judged on: the bounds, their neighbours on both sides, infinities, a NaN, both zeros."""
    c = np.float32(c)
    inf = np.float32(np.inf)
    return np.array([c, -c, np.nextafter(c, inf), np.nextafter(-c, -inf), np.nextafter(c, np.float32(0)), np.nextafter(-c, np.float32(0)),
                     inf, -inf, np.nan, -0.0, 0.0], dtype=np.float32)


def fanout_inputs(n, NM, P, K, c=UPSTREAM_CLAMP, seed=0):
    """Random planes of spread 1.5 c (about half the values beyond the bounds) with `specials` at the start, in the middle and at the very end
    of the plane array, and prompt tables whose rows all differ.  -> (low_res, coords, labels, pair_image)."""
    g = np.random.default_rng(1000 + seed + 7 * n + 13 * P)
    low = (g.standard_normal((n, NM, P)) * 1.5 * c).astype(np.float32)
    flat = low.reshape(-1)
    sp = specials(c)
    for k, v in enumerate(sp):                                               # spread over the array, wrapping in the tiny rows
        flat[k % flat.size] = v
        flat[(flat.size // 2 + k) % flat.size] = v
    flat[-1], flat[-min(2, flat.size)] = np.nan, -np.inf
    if flat.size >= 4:
        flat[0], flat[1], flat[2] = -0.0, np.nextafter(np.float32(c), np.float32(np.inf)), np.nan
    coords = g.uniform(0, 256, (n, K, 2)).astype(np.float32)
    labels = g.integers(-1, 4, (n, K)).astype(np.int32) + 10 * np.arange(n, dtype=np.int32)[:, None]      # every row its own
    pair_image = (np.arange(n, dtype=np.int32) * 3 + 1) % 5
    return low, coords, labels, pair_image


def same_bits(a, b):
    """Equality through the int32 view: NaN equals the same NaN, -0.0 differs from 0.0."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def same_fanout(got, want):
    return all((g is None and w is None) or (g is not None and w is not None and same_bits(g, w)) for g, w in zip(got, want))
