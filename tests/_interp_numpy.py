"""Vertical interpolation restated in NumPy, independently of the reference's implementation -- TEST INFRASTRUCTURE.

The reference loops over the targets and counts `coord > target` along the whole column for each.  Here every column
is brought into ascending order and its targets are placed by `numpy.searchsorted` (small problems, column by column)
or by a bisection vectorised over all (target, column) pairs (large ones); the bracketing values are gathered with
`take_along_axis` and the regions outside the column are filled by masks.  tests/test_interp_cpu.py holds it to the
recorded reference output bit for bit, so it can judge sizes that fixtures cannot hold (tests/test_gpu_interp.py).

Arithmetic dtype: f32 only when data, coord, target and the active aux arrays are all f32, f64 otherwise; the result
has data's dtype (f64 for non-floating data).
"""
import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
SEARCHSORTED_MAX = 4096  # columns: above this the vectorised bisection places the targets


def arith_dtype(*arrays):
    parts = [np.asarray(a).dtype for a in arrays if a is not None]
    return F32 if np.result_type(*parts, np.float32) == F32 else F64


def _place_searchsorted(c_desc, tc):
    """Number of levels above each target (coordinate > target) per column, [nt, n]; 0 for a column holding a NaN."""
    nlev, n = c_desc.shape
    idx = np.zeros(tc.shape, dtype=np.int64)
    asc = c_desc[::-1]
    for j in range(n):
        col = asc[:, j]
        if np.isnan(col).any():
            continue
        idx[:, j] = nlev - np.searchsorted(col, tc[:, j], side="right")  # a NaN target sorts last: 0
    return idx


def _place_bisect(c_desc, tc):
    nlev, n = c_desc.shape
    lo = np.zeros(tc.shape, dtype=np.int64)
    hi = np.full(tc.shape, nlev, dtype=np.int64)
    while True:
        open_ = lo < hi
        if not open_.any():
            return lo
        mid = (lo + hi) >> 1
        above = np.take_along_axis(c_desc, np.minimum(mid, nlev - 1), axis=0) > tc
        lo = np.where(open_ & above, mid + 1, lo)
        hi = np.where(open_ & ~above, mid, hi)


def _weight(c_top, c_bottom, tc, mode):
    if mode == "linear":
        return (tc - c_bottom) / (c_top - c_bottom)
    if mode == "log":
        return (np.log(tc) - np.log(c_bottom)) / (np.log(c_top) - np.log(c_bottom))
    one, zero = np.ones((), c_top.dtype), np.zeros((), c_top.dtype)
    return np.where(np.abs(c_top - tc) < np.abs(c_bottom - tc), one, zero)


def columns(data, coord, target, mode, aux_min=None, aux_max=None, dtype=None, descending=None, place=None):
    """data [nlev, n]; coord [nlev, n] or [nlev]; target [nt] or [nt, n]; aux_* = (data, coord), each a scalar or [n].
    Returns ([nt, n] in the arithmetic dtype, the bracket index [nt, n])."""
    T = np.dtype(dtype)
    d = np.asarray(data).astype(T, copy=False)
    nlev, n = d.shape
    c = np.asarray(coord).astype(T, copy=False)
    if c.ndim == 1:
        c = np.broadcast_to(c[:, None], (nlev, n))
    if descending is None:
        descending = not bool(c[0, 0] < c[-1, 0])
    if not descending:
        d, c = d[::-1], c[::-1]
    tc = np.asarray(target).astype(T, copy=False)
    if tc.ndim == 1:
        tc = np.broadcast_to(tc[:, None], (tc.shape[0], n))
    if place is None:
        place = _place_searchsorted if n <= SEARCHSORTED_MAX else _place_bisect
    idx = place(c, tc)
    nan = np.full((), np.nan, T)
    with np.errstate(all="ignore"):
        top = np.clip(idx, 1, nlev - 1)
        g = lambda a, i: np.take_along_axis(a, i, axis=0)  # noqa: E731
        f = _weight(g(c, top), g(c, top - 1), tc, mode)
        out = (1.0 - f) * g(d, top - 1) + f * g(d, top)
        for side, aux in ((0, aux_max), (-1, aux_min)):  # beyond the largest / the smallest coordinate
            outside = idx == 0 if side == 0 else idx == nlev
            c_end, d_end = np.broadcast_to(c[side], tc.shape), np.broadcast_to(d[side], tc.shape)
            if aux is None or aux[0] is None or aux[1] is None:
                val = d_end if mode == "nearest" else np.where(np.isclose(c_end, tc), d_end, nan)
            else:
                ad = np.broadcast_to(np.asarray(aux[0]).astype(T, copy=False).reshape(-1), (n,))
                ac = np.broadcast_to(np.asarray(aux[1]).astype(T, copy=False).reshape(-1), (n,))
                ad, ac = np.broadcast_to(ad, tc.shape), np.broadcast_to(ac, tc.shape)
                if side == 0:
                    ok = (ac > c_end) & (ac >= tc)
                    f = _weight(c_end, ac, tc, mode)
                    val = np.where(ok, (1.0 - f) * ad + f * d_end, nan)
                else:
                    ok = (ac < c_end) & (ac <= tc)
                    f = _weight(ac, c_end, tc, mode)
                    val = np.where(ok, (1.0 - f) * d_end + f * ad, nan)
            out = np.where(outside, val, out)
    return out.astype(T, copy=False), idx


def _result_dtype(data):
    dt = np.asarray(data).dtype
    return dt if dt.kind == "f" else F64


def monotonic(data, coord, target_coord, interpolation="linear", aux_min_level_data=None, aux_min_level_coord=None,
              aux_max_level_data=None, aux_max_level_coord=None, vertical_axis=0, place=None):
    data, coord, target = np.asarray(data), np.atleast_1d(coord), np.atleast_1d(target_coord)
    if vertical_axis != 0:
        data, coord, target = (np.moveaxis(x, vertical_axis, 0) if x.ndim > 1 else x for x in (data, coord, target))
    aux_min, aux_max = (aux_min_level_data, aux_min_level_coord), (aux_max_level_data, aux_max_level_coord)
    if coord.shape != data.shape:  # a level vector against fields: no aux layers there
        aux_min = aux_max = None
    active = [x for a in (aux_min, aux_max) if a is not None and a[0] is not None and a[1] is not None for x in a]
    T = arith_dtype(data.astype(_result_dtype(data), copy=False), coord, target, *active)
    cols = data.shape[1:]
    n = int(np.prod(cols, dtype=np.int64))
    flat = lambda x: None if x is None else (np.broadcast_to(x, cols).reshape(-1) if np.size(x) != 1 else np.reshape(x, -1))  # noqa: E731
    out, _ = columns(data.reshape(data.shape[0], n), coord if coord.ndim == 1 and data.ndim > 1 else coord.reshape(coord.shape[0], n),
                     target if target.ndim == 1 else target.reshape(target.shape[0], n), interpolation,
                     None if aux_min is None else tuple(flat(x) for x in aux_min),
                     None if aux_max is None else tuple(flat(x) for x in aux_max), dtype=T, place=place)
    out = out.reshape((target.shape[0],) + cols).astype(_result_dtype(data), copy=False)
    if vertical_axis != 0 and out.ndim > 1:
        out = np.moveaxis(out, 0, vertical_axis)
    return out


def hybrid_pressure(A, B, sp, nlev, dtype):
    """p on the bottom-most `nlev` full levels of the table, [nlev, *sp.shape], every operation rounded in `dtype`."""
    A, B = np.asarray(A).astype(dtype)[len(A) - 1 - nlev:], np.asarray(B).astype(dtype)[len(B) - 1 - nlev:]
    sp = np.asarray(sp).astype(dtype)
    shape = (-1,) + (1,) * sp.ndim
    with np.errstate(all="ignore"):
        half = A.reshape(shape) + B.reshape(shape) * sp[None]
        return half[:-1] + 0.5 * (half[1:] - half[:-1])


def hybrid_to_pressure(data, target_p, A, B, sp, alpha_top="ifs", interpolation="linear", aux_bottom_data=None,
                       aux_bottom_p=None, aux_top_data=None, aux_top_p=None, vertical_axis=0, place=None):
    data, target = np.asarray(data), np.atleast_1d(target_p)
    if vertical_axis != 0:
        data, target = (np.moveaxis(x, vertical_axis, 0) if x.ndim > 1 else x for x in (data, target))
    active = [x for a in ((aux_bottom_data, aux_bottom_p), (aux_top_data, aux_top_p)) if a[0] is not None and a[1] is not None for x in a]
    T = arith_dtype(data.astype(_result_dtype(data), copy=False), target, A, B, sp, *active)
    p = hybrid_pressure(A, B, np.broadcast_to(sp, data.shape[1:]), data.shape[0], T)
    # the arithmetic dtype is passed on through the coordinate (an f64 coordinate makes everything f64)
    out = monotonic(data, p, target.astype(T), interpolation, aux_top_data, aux_top_p, aux_bottom_data, aux_bottom_p, 0, place)
    if vertical_axis != 0 and out.ndim > 1:
        out = np.moveaxis(out, 0, vertical_axis)
    return out


def height_from_geopotential(z, zs, h_type="geometric", h_reference="ground"):
    """The height coordinate of pressure levels, every operation rounded in the promotion of z and zs."""
    z, zs = np.asarray(z), np.asarray(zs)
    g, re = 9.80665, 6371229
    with np.errstate(all="ignore"):
        if h_type == "geometric":
            zz = z / g
            h = re * zz / (re - zz)
            if h_reference == "ground":
                zzs = zs / g
                h = h - re * zzs / (re - zzs)
            return h
        return (z - zs if h_reference == "ground" else z) / g


def pressure_to_height(data, target_h, z, zs, h_type="geometric", h_reference="ground", interpolation="linear",
                       aux_bottom_data=None, aux_bottom_h=None, aux_top_data=None, aux_top_h=None, vertical_axis=0, place=None):
    h = height_from_geopotential(z, zs, h_type, h_reference)
    return monotonic(data, h, target_h, interpolation, aux_bottom_data, aux_bottom_h, aux_top_data, aux_top_h, vertical_axis, place)


def same_bits(a, b):
    """Equal dtype, shape, NaN positions and bits everywhere else."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(f"u{a.dtype.itemsize}"), b[~nb].view(f"u{a.dtype.itemsize}")))
