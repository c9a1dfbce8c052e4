"""`earthkit.meteo.vertical.pressure_on_hybrid_levels` on MI355X -- the producer of the
model-level pressure field the thermo kernels consume.

Same signature, outputs, level selection/ordering and error messages as the reference
(/root/reference/src/earthkit/meteo/vertical/array/vertical.py:505-740).  NumPy `sp` in ->
NumPy out; `DeviceArray` `sp` in -> DeviceArrays out (then `vertical_axis` must be 0).
`HybridPressure(A, B, sp)` hands the same definition to the thermo kernels instead of a
materialised pressure field (ekm_hip.thermo functions accept it in place of `p`).
"""
import ctypes as C
import math

import numpy as np

from . import _ffi
from .device import DeviceArray, _Allocation, current_device, current_stream

_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
PRESSURE_TOA = 0.1  # vertical.py:674


def _foreign_aware(*names):
    """Arguments `names` of the wrapped function may be arrays of another ROCm library (torch / cupy device tensors:
    `__dlpack_device__()` says kDLROCM): they are taken over through DLPack exactly as in ekm_hip.thermo
    (`_engine._adopt_foreign`), and when every such argument came from one library the DeviceArray results go back
    through that library's `from_dlpack`."""
    import functools
    import inspect

    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            from . import _engine

            bound = sig.bind(*args, **kwargs)
            present = [n for n in names if n in bound.arguments and bound.arguments[n] is not None]
            adopted, module = _engine._adopt_foreign([bound.arguments[n] for n in present])
            for n, a in zip(present, adopted):
                bound.arguments[n] = a
            res = fn(*bound.args, **bound.kwargs)
            if module is None:
                return res
            out = _engine._hand_back(res if isinstance(res, tuple) else (res,), module)
            return out if isinstance(res, tuple) else out[0]

        wrapper.__signature__ = sig
        return wrapper

    return deco


def _dev_bytes(host_array, device):
    a = np.ascontiguousarray(host_array)
    alloc = _Allocation(max(a.nbytes, 16), device)
    lib = _ffi.lib()
    _ffi.check(lib.ekm_h2d(device, alloc.ptr, a.ctypes.data, a.nbytes, current_stream()))
    _ffi.check(lib.ekm_stream_sync(device, current_stream()))
    return alloc


def _compute_dtype(A, B, sp):
    parts = [x.dtype for x in (A, B, sp)]
    rd = np.result_type(*parts, 0.0)
    return _F32 if rd == _F32 else _F64


def _select_levels(A, B, levels):
    """vertical.py:641-661: contiguous half-level range covering the request + row maps."""
    nlev = A.shape[0] - 1
    levels = np.asarray(levels)
    lmax, lmin = int(levels.max()), int(levels.min())
    if lmax > nlev:
        raise ValueError(f"Requested level {lmax} exceeds the maximum number of levels {nlev}.")
    if lmin < 1:
        raise ValueError(f"Level numbering starts at 1. Found level={lmin} < 1.")
    half_idx = np.arange(lmin - 1, lmax + 1)
    out_half_idx = np.nonzero(levels[:, None] == half_idx[None, :])[1]  # local half index per requested level
    return A[half_idx], B[half_idx], out_half_idx


@_foreign_aware("sp")
def pressure_on_hybrid_levels(A, B, sp, levels=None, alpha_top="ifs", output="full", vertical_axis=0):
    """Pressure on hybrid full/half levels and the delta/alpha layer parameters (vertical.py:505-740)."""
    if isinstance(output, str):
        output = (output,)
    if not output:
        raise ValueError("At least one output type must be specified.")
    for out in output:
        if out not in ["full", "half", "alpha", "delta"]:
            raise ValueError(f"Unknown output type '{out}'. Allowed values are 'full', 'half', 'alpha' or 'delta'.")
    if alpha_top not in ["ifs", "arpege"]:
        raise ValueError(f"Unknown method '{alpha_top}' for pressure calculation. Use 'ifs' or 'arpege'.")

    A = np.asarray(A)
    B = np.asarray(B)
    on_device = isinstance(sp, DeviceArray)
    if not on_device:
        sp = np.asarray(sp)
    if on_device and vertical_axis != 0 and sp.ndim > 0:
        raise ValueError("DeviceArray input: outputs are level-major, vertical_axis must be 0")
    dtype = _compute_dtype(A, B, sp)
    device = sp.device if on_device else current_device()

    sel = None
    if levels is not None:
        A, B, sel = _select_levels(A, B, levels)
    nfull = A.shape[0] - 1
    sp_shape = tuple(sp.shape)
    npts = int(math.prod(sp_shape))

    # output rows: identity, or the requested levels in the requested order
    if sel is None:
        nrow_full, nrow_half, row_full, row_half = nfull, nfull + 1, None, None
        dup = None
    else:
        uniq, first = np.unique(sel, return_index=True)
        dup = None if len(uniq) == len(sel) else sel  # repeated levels: compute unique rows, then gather
        order = uniq if dup is not None else sel
        row_half = np.full(nfull + 1, -1, np.int32)
        row_half[order] = np.arange(len(order), dtype=np.int32)
        row_full = np.full(nfull, -1, np.int32)
        row_full[order - 1] = np.arange(len(order), dtype=np.int32)
        nrow_full = nrow_half = len(order)

    lib = _ffi.lib()
    stream = current_stream()
    tag, real = ("f32", C.c_float) if dtype == _F32 else ("f64", C.c_double)
    d_sp = sp if (on_device and sp.dtype == dtype) else DeviceArray.from_host(np.asarray(sp, dtype=dtype), device)
    d_a = DeviceArray.from_host(A.astype(dtype), device)
    d_b = DeviceArray.from_host(B.astype(dtype), device)
    d_rf = _dev_bytes(row_full, device) if row_full is not None else None
    d_rh = _dev_bytes(row_half, device) if row_half is not None else None

    d_sp.on(stream)  # an `sp` last used on another stream: order this stream after that work
    top_is_zero = _top_is_zero(A[0], B[0], sp, d_sp, dtype, npts, device, on_device)
    a_top = float(np.log(2)) if alpha_top == "ifs" else 1.0

    bufs = {}
    for name in set(output):
        rows = nrow_half if name == "half" else nrow_full
        bufs[name] = DeviceArray.empty((rows,) + sp_shape, dtype, device)
    ptr = lambda n: bufs[n].ptr if n in bufs else None  # noqa: E731
    _ffi.check(getattr(lib, f"ekm_pressure_on_hybrid_levels_{tag}")(
        device, stream, d_a.ptr, d_b.ptr, d_sp.ptr, npts, nfull, d_rf.ptr if d_rf else None,
        d_rh.ptr if d_rh else None, int(top_is_zero), real(a_top), ptr("full"), ptr("half"), ptr("delta"),
        ptr("alpha")))

    res = []
    if on_device:
        _ffi.check(lib.ekm_stream_sync(device, stream))
        for name in output:
            arr = bufs[name]
            if dup is not None:  # repeated levels: gather rows device-to-device
                uniq = np.unique(dup)
                out = DeviceArray.empty((len(dup),) + sp_shape, dtype, device)
                row_bytes = npts * dtype.itemsize
                for r, h in enumerate(dup):
                    src = int(np.searchsorted(uniq, h))
                    _ffi.check(lib.ekm_d2d(device, out.ptr + r * row_bytes, arr.ptr + src * row_bytes, row_bytes, stream))
                _ffi.check(lib.ekm_stream_sync(device, stream))
                arr = out
            res.append(arr)
    else:
        for name in output:
            h = bufs[name].to_host()
            if dup is not None:
                h = h[np.searchsorted(np.unique(dup), dup)]
            if name in ("delta", "alpha") and h.dtype != _F64:
                h = h.astype(np.float64)  # the reference allocates these with the default dtype (vertical.py:678, 687)
            res.append(h)
        for b in bufs.values():
            b.free()
        if vertical_axis != 0 and res[0].ndim > 1:
            res = [np.moveaxis(r, 0, vertical_axis) for r in res]
    return res[0] if len(res) == 1 else tuple(res)


def _top_is_zero(A0, B0, sp, d_sp, dtype, npts, device, on_device):
    """The reference's global any(p_half[0] <= 0.1) (vertical.py:680, 694)."""
    lib, stream = _ffi.lib(), current_stream()
    a0, b0 = float(A0), float(B0)
    if b0 == 0.0 or npts == 0:
        return bool(a0 <= PRESSURE_TOA)
    if not on_device:
        return bool(np.any(np.asarray(A0, dtype) + np.asarray(B0, dtype) * np.asarray(sp, dtype=dtype) <= PRESSURE_TOA))
    tag, real = ("f32", C.c_float) if dtype == _F32 else ("f64", C.c_double)
    flag = _dev_bytes(np.zeros(1, np.int32), device)
    _ffi.check(getattr(lib, f"ekm_any_le_{tag}")(device, stream, d_sp.ptr, npts, real(a0), real(b0),
                                                 real(PRESSURE_TOA), flag.ptr))
    host = np.zeros(1, np.int32)
    _ffi.check(lib.ekm_d2h(device, host.ctypes.data, flag.ptr, 4, stream))
    _ffi.check(lib.ekm_stream_sync(device, stream))
    return bool(host[0])


_GEO_MODE = {"thickness": 0, "geopotential": 1, ("geometric", "sea"): 2, ("geopotential", "sea"): 3,
             ("geometric", "ground"): 4, ("geopotential", "ground"): 5}


def _chain(t, q, zs, A, B, sp, alpha_top, mode, vertical_axis, device_result=False):
    """t, q on hybrid full levels + surface pressure -> geopotential thickness / geopotential / height in
    ONE bottom-up pass per column (vertical.py:741-1190); alpha, delta and the half-level pressures are
    formed on the fly and never stored.  `device_result`: the level-major field stays in device memory whatever the
    inputs were (it feeds the interpolation kernel), rounded to the dtype a NumPy caller would have got."""
    if alpha_top not in ["ifs", "arpege"]:
        raise ValueError(f"Unknown method '{alpha_top}' for pressure calculation. Use 'ifs' or 'arpege'.")
    A, B = np.asarray(A), np.asarray(B)
    arrs = dict(t=t, q=q, sp=sp, zs=zs)
    on_device = any(isinstance(v, DeviceArray) for v in arrs.values())
    if on_device and vertical_axis != 0:
        raise ValueError("DeviceArray input: fields are level-major, vertical_axis must be 0")
    host = {k: (v if isinstance(v, DeviceArray) else (None if v is None else np.asarray(v))) for k, v in arrs.items()}
    if not on_device and vertical_axis != 0:
        host["t"], host["q"] = (np.moveaxis(host[k], vertical_axis, 0) for k in ("t", "q"))
    parts = [v.dtype for v in host.values() if v is not None] + [A.dtype, B.dtype]
    dtype = _F32 if np.result_type(*parts, 0.0) == _F32 else _F64
    out_parts = [host["t"].dtype, host["q"].dtype] + ([host["zs"].dtype] if zs is not None and mode not in (0, 5) else [])
    out_dtype = np.result_type(*out_parts, np.float32 if all(p == _F32 for p in out_parts) else 0.0)
    if not on_device and host["t"].ndim >= 1:
        # NumPy input broadcasts as it does in the reference (t of [levels, 1] against q and sp of [.., n]): the level count is
        # t's (vertical.py:1191-1203), everything is brought to [levels, *columns] on the host
        try:
            full = np.broadcast_shapes(host["t"].shape, host["q"].shape, (host["t"].shape[0],) + tuple(host["sp"].shape))
            if full[0] == host["t"].shape[0] and (host["zs"] is None or np.broadcast_shapes(full[1:], host["zs"].shape) == full[1:]):
                host["t"], host["q"] = np.broadcast_to(host["t"], full), np.broadcast_to(host["q"], full)
                host["sp"] = np.broadcast_to(host["sp"], full[1:])
                if host["zs"] is not None:
                    host["zs"] = np.broadcast_to(host["zs"], full[1:])
        except ValueError:
            pass  # not broadcastable: the shape error below
    shape = tuple(host["t"].shape)
    if tuple(host["q"].shape) != shape or shape[1:] != tuple(host["sp"].shape):
        raise ValueError(f"t {shape}, q {tuple(host['q'].shape)} must be [levels, *sp.shape] with sp {tuple(host['sp'].shape)}")
    nlev_t, nlev = shape[0], A.shape[0] - 1
    if nlev_t > nlev:
        raise ValueError(f"data have {nlev_t} levels, A/B have {nlev} levels")
    A, B = A[nlev - nlev_t:], B[nlev - nlev_t:]  # the bottom-most nlev_t layers (vertical.py:1191-1203)
    npts = int(math.prod(shape[1:]))
    device = next((v.device for v in host.values() if isinstance(v, DeviceArray)), current_device())

    def dev(v):
        if isinstance(v, DeviceArray) and v.dtype == dtype:
            return v
        return DeviceArray.from_host(np.ascontiguousarray(np.asarray(v), dtype=dtype), device)

    d = {k: (dev(v) if v is not None else None) for k, v in host.items()}
    for v in d.values():
        if v is not None:
            v.on(current_stream())  # inputs last used on another stream: order this stream after that work
    d_a, d_b = dev(A), dev(B)
    top = _top_is_zero(A[0], B[0], host["sp"], d["sp"], dtype, npts, device, isinstance(host["sp"], DeviceArray))
    a_top = float(np.log(2)) if alpha_top == "ifs" else 1.0
    out = DeviceArray.empty(shape, dtype, device)
    lib = _ffi.lib()
    tag, real = ("f32", C.c_float) if dtype == _F32 else ("f64", C.c_double)
    _ffi.check(getattr(lib, f"ekm_geopotential_on_hybrid_levels_{tag}")(
        device, current_stream(), d_a.ptr, d_b.ptr, d["sp"].ptr, d["zs"].ptr if d["zs"] is not None else None,
        d["t"].ptr, d["q"].ptr, npts, nlev_t, int(top), real(a_top), mode, out.ptr))
    if on_device:
        _ffi.check(lib.ekm_stream_sync(device, current_stream()))
        return out
    if device_result and out_dtype == dtype:
        return out
    res = out.to_host().astype(out_dtype, copy=False)
    out.free()
    if device_result:  # mixed dtypes: the field a NumPy caller gets is rounded to t's and q's dtype
        return DeviceArray.from_host(res, device)
    if vertical_axis != 0:
        res = np.moveaxis(res, 0, vertical_axis)
    return res


@_foreign_aware("t", "q", "alpha", "delta")
def relative_geopotential_thickness_on_hybrid_levels_from_alpha_delta(t, q, alpha, delta, vertical_axis=0):
    """Geopotential thickness between the surface and the hybrid full levels from alpha and delta the caller
    already holds (outputs of `pressure_on_hybrid_levels`): vertical.py:741-893.  The same bottom-up column scan
    as `relative_geopotential_thickness_on_hybrid_levels`, with alpha and delta STREAMED (16 B read + 4 B written
    per point in fp32) instead of formed from A, B, sp.  NumPy result dtype = that of t and q, as in the reference."""
    arrs = dict(t=t, q=q, alpha=alpha, delta=delta)
    on_device = any(isinstance(v, DeviceArray) for v in arrs.values())
    if on_device and vertical_axis != 0:
        raise ValueError("DeviceArray input: fields are level-major, vertical_axis must be 0")
    host = {k: (v if isinstance(v, DeviceArray) else np.asarray(v)) for k, v in arrs.items()}
    if vertical_axis != 0:
        host = {k: np.moveaxis(v, vertical_axis, 0) for k, v in host.items()}
    # the reference writes into zeros_like(R(q) * t) (vertical.py:762): the RESULT has the dtype of t and q, while the
    # arithmetic runs in the promotion of all four (its own alpha / delta are fp64 whatever the input dtype)
    out_dtype = np.result_type(host["t"].dtype, host["q"].dtype)
    if out_dtype.kind != "f":
        out_dtype = _F64
    cd = np.result_type(*[v.dtype for v in host.values()])
    dtype = _F32 if cd in (_F32, np.dtype(np.float16)) else _F64
    shape = tuple(host["t"].shape)
    if len(shape) == 0 or any(tuple(v.shape) != shape for v in host.values()):
        raise ValueError("t, q, alpha and delta must have the same shape [levels, ...]: "
                         + ", ".join(f"{k} {tuple(v.shape)}" for k, v in host.items()))
    nlev, npts = shape[0], int(math.prod(shape[1:]))
    device = next((v.device for v in host.values() if isinstance(v, DeviceArray)), current_device())
    stream = current_stream()
    d = {}
    for k, v in host.items():
        d[k] = v if isinstance(v, DeviceArray) and v.dtype == dtype else DeviceArray.from_host(
            np.ascontiguousarray(np.asarray(v), dtype=dtype), device)
        d[k].on(stream)
    out = DeviceArray.empty(shape, dtype, device)
    lib = _ffi.lib()
    tag = "f32" if dtype == _F32 else "f64"
    _ffi.check(getattr(lib, f"ekm_geopotential_thickness_from_alpha_delta_{tag}")(
        device, stream, d["t"].ptr, d["q"].ptr, d["alpha"].ptr, d["delta"].ptr, npts, nlev, out.on(stream)))
    if on_device:
        return out  # device-resident: in the arithmetic dtype
    res = out.to_host().astype(out_dtype, copy=False)
    out.free()
    if vertical_axis != 0:
        res = np.moveaxis(res, 0, vertical_axis)
    return res


@_foreign_aware("t", "q", "sp")
def relative_geopotential_thickness_on_hybrid_levels(t, q, A, B, sp, alpha_top="ifs", vertical_axis=0):
    """Geopotential thickness between the surface and the hybrid full levels (vertical.py:894-994)."""
    return _chain(t, q, None, A, B, sp, alpha_top, _GEO_MODE["thickness"], vertical_axis)


@_foreign_aware("t", "q", "zs", "sp")
def geopotential_on_hybrid_levels(t, q, zs, A, B, sp, alpha_top="ifs", vertical_axis=0):
    """Geopotential on hybrid full levels (vertical.py:997-1069)."""
    return _chain(t, q, zs, A, B, sp, alpha_top, _GEO_MODE["geopotential"], vertical_axis)


@_foreign_aware("t", "q", "zs", "sp")
def height_on_hybrid_levels(t, q, zs, A, B, sp, alpha_top="ifs", h_type="geometric", h_reference="ground",
                            vertical_axis=0):
    """Geometric / geopotential height above sea level / ground on hybrid full levels (vertical.py:1072-1188)."""
    if h_reference not in ["sea", "ground"]:
        raise ValueError(f"Unknown '{h_reference=}'. Use 'sea' or 'ground'.")
    key = ("geometric" if h_type == "geometric" else "geopotential", h_reference)
    return _chain(t, q, zs, A, B, sp, alpha_top, _GEO_MODE[key], vertical_axis)


# ---- vertical interpolation (vertical/array/vertical.py:1206-1719, vertical/array/monotonic.py) ----
_INTERP_MODE = {"linear": 0, "log": 1, "nearest": 2}


def _arith_dtype(parts):
    """f32 only when every array taking part is f32, f64 otherwise (NumPy promotion of data, coord, target and aux)."""
    return _F32 if np.result_type(*parts, np.float32) == _F32 else _F64


def _to_device(x, dtype, device, shape=None):
    """`x` (DeviceArray or NumPy) as a contiguous DeviceArray of `dtype`; a DeviceArray of another dtype goes through the host."""
    if isinstance(x, DeviceArray):
        if x.dtype == dtype:
            return x
        x = x.to_host()
    x = np.asarray(x, dtype=dtype)
    if shape is not None:
        x = np.broadcast_to(x, shape)
    return DeviceArray.from_host(np.ascontiguousarray(x), device)


def _interp_check(interpolation, data, coord_shape, target, vertical_axis, on_device):
    """The argument checks of monotonic.py:63-122 on shapes alone (no device call): returns (nlev, columns shape)."""
    if interpolation not in _INTERP_MODE:
        raise ValueError(f"Unknown interpolation method '{interpolation}'. Supported methods are 'linear', 'log' and 'nearest'.")
    if on_device and vertical_axis != 0:
        raise ValueError("DeviceArray input: fields are level-major, vertical_axis must be 0")
    dshape, tshape = tuple(data.shape), tuple(target.shape)
    if len(dshape) == 0 or dshape[0] < 2:
        raise ValueError("At least two levels are required for interpolation.")
    if dshape[0] != coord_shape[0]:
        raise ValueError(f"The first dimension of data and that of coord must match! {dshape=} {coord_shape=}")
    same = dshape == tuple(coord_shape)
    if same:
        if len(dshape) == 1 and len(tshape) != 1:
            raise ValueError("If values and p have the same shape, they cannot both be scalars.")
        if len(dshape) > 1 and len(tshape) != 1 and dshape[1:] != tshape[1:]:
            raise ValueError("When values and target_p have different shapes, target_p must be a scalar or a 1D array.")
    elif len(coord_shape) != 1:
        raise ValueError(f"When values and p have different shapes, p must be a scalar or a 1D array. {dshape=} {coord_shape=}")
    elif len(tshape) != 1 and (dshape[-1] != dshape[0] or dshape[1:] != tshape[1:]):
        # the reference broadcasts the level vector along the LAST axis and transposes (monotonic.py:143): that works
        # only where the last axis is as long as the level axis, and fails to broadcast everywhere else
        raise ValueError("A 1D coord needs a scalar or 1D target_coord (or data whose last axis is as long as its level axis).")
    return dshape[0], dshape[1:]


def _interp_run(data, target, interpolation, aux, descending, dtype, out_dtype, device, cols, coord=None, hybrid=None):
    """Upload what is not on the device yet, launch the generic kernel (`coord`) or the fused hybrid->pressure one
    (`hybrid` = (A, B, sp)), and hand the [ntarget, *cols] result back as a DeviceArray of the arithmetic dtype."""
    nlev, npts = int(data.shape[0]), int(math.prod(cols))
    stream = current_stream()
    keep = []  # device buffers of this call: alive until the launch is enqueued

    def dev(x, shape=None):
        d = _to_device(x, dtype, device, shape)
        d.on(stream)
        keep.append(d)
        return d

    d_data = dev(data)
    t_field = len(target.shape) != 1
    d_target = dev(target)
    ntarget = int(target.shape[0])
    ptrs, mask = [], 0
    for e, (ad, ac) in enumerate(aux):  # (min_data, min_coord), (max_data, max_coord)
        if ad is None or ac is None:
            ptrs += [None, None]
            continue
        for b, x in enumerate((ad, ac)):
            size = int(math.prod(x.shape)) if isinstance(x, DeviceArray) else np.size(x)
            if size == 1:
                ptrs.append(dev(x if isinstance(x, DeviceArray) else np.reshape(x, (1,))).ptr)
            else:
                if isinstance(x, DeviceArray) and tuple(x.shape) != tuple(cols):
                    raise ValueError(f"aux array of shape {tuple(x.shape)} does not match a level of data {tuple(cols)}")
                ptrs.append(dev(x, cols).ptr)
                mask |= 1 << (2 * e + b)
    out = DeviceArray.empty((ntarget,) + tuple(cols), dtype, device)
    lib = _ffi.lib()
    tag = "f32" if dtype == _F32 else "f64"
    mode = _INTERP_MODE[interpolation]
    if hybrid is not None:
        d_a, d_b, d_sp = (dev(x) for x in hybrid)
        _ffi.check(getattr(lib, f"ekm_interpolate_hybrid_to_pressure_{tag}")(
            device, stream, d_data.ptr, d_a.ptr, d_b.ptr, d_sp.ptr, d_target.ptr, int(t_field), ntarget, npts, nlev,
            int(descending), mode, ptrs[0], ptrs[1], ptrs[2], ptrs[3], mask, out.on(stream)))
    else:
        c_field = len(coord.shape) != 1 or npts == 1 and len(cols) == 0
        d_coord = dev(coord)
        _ffi.check(getattr(lib, f"ekm_interpolate_monotonic_{tag}")(
            device, stream, d_data.ptr, d_coord.ptr, int(c_field), d_target.ptr, int(t_field), ntarget, npts, nlev,
            int(descending), mode, ptrs[0], ptrs[1], ptrs[2], ptrs[3], mask, out.on(stream)))
    return out


def _interp_finish(out, on_device, out_dtype, vertical_axis):
    if on_device:
        return out
    res = out.to_host().astype(out_dtype, copy=False)
    out.free()
    if vertical_axis != 0 and res.ndim > 1:
        res = np.moveaxis(res, 0, vertical_axis)
    return res


def _host_or_dev(x, atleast_1d=False):
    if x is None or isinstance(x, DeviceArray):
        return x
    return np.atleast_1d(x) if atleast_1d else np.asarray(x)


def _first_two_ends(coord, device):
    """coord[0] and coord[-1] of the first column (monotonic.py:84-89); two elements read back for a DeviceArray."""
    if not isinstance(coord, DeviceArray):
        flat = coord.reshape(coord.shape[0], -1)
        return flat[0, 0], flat[-1, 0]
    lib, stream = _ffi.lib(), current_stream()
    coord.on(stream)
    host = np.zeros(2, coord.dtype)
    row = int(math.prod(coord.shape[1:])) * coord.dtype.itemsize
    item = coord.dtype.itemsize
    _ffi.check(lib.ekm_d2h(device, host.ctypes.data, coord.ptr, item, stream))
    _ffi.check(lib.ekm_d2h(device, host.ctypes.data + item, coord.ptr + (coord.shape[0] - 1) * row, item, stream))
    _ffi.check(lib.ekm_stream_sync(device, stream))
    return host[0], host[1]


def _out_dtype(data):
    """The result has data's dtype; non-floating data is computed and returned in f64 (the reference writes NaN into an
    integer array there: the one typing deviation)."""
    return np.dtype(data.dtype) if np.dtype(data.dtype) in (_F32, _F64, np.dtype(np.float16)) else _F64


@_foreign_aware("data", "coord", "target_coord", "aux_min_level_data", "aux_min_level_coord", "aux_max_level_data",
                "aux_max_level_coord")
def interpolate_monotonic(data, coord, target_coord, interpolation="linear", aux_min_level_data=None,
                          aux_min_level_coord=None, aux_max_level_data=None, aux_max_level_coord=None, vertical_axis=0):
    """Interpolate `data` between levels of a monotonic coordinate (vertical.py:1616-1719, monotonic.py:49-370):
    'linear', 'log' or 'nearest', NaN outside the column unless an aux layer reaches the target.

    NumPy in -> NumPy out; DeviceArray in -> DeviceArray out (level-major, `vertical_axis` must be 0).  The arithmetic
    runs in f32 when data, coord, target_coord and the aux arrays are all f32 and in f64 otherwise.  A NumPy result has
    `data`'s dtype, except that non-floating data gives f64 (the reference writes NaN into an integer array there).
    A DeviceArray result stays in the ARITHMETIC dtype (f32 data with an f64 coord gives f64), as the device results of
    the other `vertical` functions do: the second typing deviation.  A DeviceArray argument of another dtype than the
    arithmetic one is converted on the host, which makes the call wait for the device.
    The ordering of the levels is read from the first column, as in the reference; nothing is flipped in memory.
    With a 1D `coord`, multi-dimensional `data` and a scalar or 1D target the aux layers are not used
    (monotonic.py:299-358).  A 1D `coord` with a multi-dimensional target raises ValueError where the reference fails to
    broadcast it (monotonic.py:143), which is everywhere except where data's last axis is as long as its level axis;
    there the coordinate is the level vector of every column, as in the reference.
    `vertical_axis` != 0 has its documented meaning in every case: the result's level axis is moved back, also for a 1D
    `coord` with a 1D target, where the reference returns the levels on axis 0 (monotonic.py:167-170)."""
    return _monotonic(data, coord, target_coord, interpolation, aux_min_level_data, aux_min_level_coord, aux_max_level_data,
                      aux_max_level_coord, vertical_axis)


def _monotonic(data, coord, target_coord, interpolation, aux_min_level_data, aux_min_level_coord, aux_max_level_data,
               aux_max_level_coord, vertical_axis, on_device=None):
    """`interpolate_monotonic`; `on_device` says what the caller was given when `coord` is a device-resident temporary of
    its own (level-major already) beside NumPy arguments."""
    data = _host_or_dev(data)
    coord = _host_or_dev(coord, True)
    target = _host_or_dev(target_coord, True)
    aux = [_host_or_dev(x, True) for x in (aux_min_level_data, aux_min_level_coord, aux_max_level_data, aux_max_level_coord)]
    if on_device is None:
        on_device = any(isinstance(x, DeviceArray) for x in [data, coord, target] + aux)
    if interpolation in _INTERP_MODE and not on_device and vertical_axis != 0:
        data, coord, target = (x if isinstance(x, DeviceArray) or x.ndim <= 1 else np.moveaxis(x, vertical_axis, 0)
                               for x in (data, coord, target))
    nlev, cols = _interp_check(interpolation, data, tuple(coord.shape), target, vertical_axis, on_device)
    if tuple(coord.shape) != tuple(data.shape) and len(target.shape) == 1:
        aux = [None] * 4  # 1D coord, 1D target, fields of data: the reference's simple_compute knows no aux layers
    aux = [(aux[0], aux[1]), (aux[2], aux[3])]
    aux = [(d, c) if d is not None and c is not None else (None, None) for d, c in aux]
    parts = [x.dtype for x in [data, coord, target] + [x for pair in aux for x in pair] if x is not None]
    out_dtype = _out_dtype(data)
    dtype = _arith_dtype(parts + [out_dtype])
    device = next((x.device for x in [data, coord, target] if isinstance(x, DeviceArray)), current_device())
    c0, c1 = _first_two_ends(coord, device)
    out = _interp_run(data, target, interpolation, aux, not bool(c0 < c1), dtype, out_dtype, device, cols, coord=coord)
    return _interp_finish(out, on_device, out_dtype, vertical_axis)


@_foreign_aware("data", "target_p", "sp", "aux_bottom_data", "aux_bottom_p", "aux_top_data", "aux_top_p")
def interpolate_hybrid_to_pressure_levels(data, target_p, A, B, sp, alpha_top="ifs", interpolation="linear",
                                          aux_bottom_data=None, aux_bottom_p=None, aux_top_data=None, aux_top_p=None,
                                          vertical_axis=0):
    """Interpolate `data` from hybrid full levels to pressure levels (vertical.py:1206-1326) in ONE kernel: the pressure
    of the model levels is formed from A, B and `sp` inside it (each operation rounded as the reference rounds it) and
    never stored.  `data` may hold fewer levels than the tables: the bottom-most ones (vertical.py:1191-1203).

    NumPy in -> NumPy out, with `vertical_axis` meaning what the reference documents (the axis is moved in and back;
    the reference itself raises a shape error there for multi-dimensional data).  DeviceArray in -> DeviceArray out,
    level-major; with `sp` on the device the call ASSUMES that pressure increases with the level index (true for every
    table whose half-level pressures do) instead of reading the first column back, so the call enqueues without a host
    wait -- provided every DeviceArray argument has the arithmetic dtype (one of another dtype is converted on the host).
    Dtypes as in `interpolate_monotonic`, with A, B and sp taking part in the promotion."""
    if alpha_top not in ["ifs", "arpege"]:
        raise ValueError(f"Unknown method '{alpha_top}' for pressure calculation. Use 'ifs' or 'arpege'.")
    A, B = np.asarray(A), np.asarray(B)
    data = _host_or_dev(data)
    sp = _host_or_dev(sp)
    target = _host_or_dev(target_p, True)
    # aux_bottom_* lies at the largest pressure (aux_max_level_*), aux_top_* at the smallest (vertical.py:1316-1326)
    aux = [_host_or_dev(x, True) for x in (aux_top_data, aux_top_p, aux_bottom_data, aux_bottom_p)]
    on_device = any(isinstance(x, DeviceArray) for x in [data, sp, target] + aux)
    if interpolation in _INTERP_MODE and not on_device and vertical_axis != 0:
        data, target = (np.moveaxis(x, vertical_axis, 0) if x.ndim > 1 else x for x in (data, target))
    nlev_t, cols = _interp_check(interpolation, data, tuple(data.shape), target, vertical_axis, on_device)
    nlev = A.shape[0] - 1
    if A.ndim != 1 or A.shape != B.shape or nlev_t > nlev:
        raise ValueError(f"data have {nlev_t} levels, A/B have {nlev} levels")
    A, B = A[nlev - nlev_t:], B[nlev - nlev_t:]
    if isinstance(sp, DeviceArray):
        if tuple(sp.shape) != tuple(cols) and not (sp.size == 1 and math.prod(cols) == 1):
            raise ValueError(f"sp {tuple(sp.shape)} does not match a level of data {tuple(cols)}")
    else:
        sp = np.broadcast_to(sp, cols)  # ValueError when it cannot
    aux = [(aux[0], aux[1]), (aux[2], aux[3])]
    aux = [(d, c) if d is not None and c is not None else (None, None) for d, c in aux]
    parts = [x.dtype for x in [data, sp, target, A, B] + [x for pair in aux for x in pair] if x is not None]
    out_dtype = _out_dtype(data)
    dtype = _arith_dtype(parts + [out_dtype])
    device = next((x.device for x in [data, sp, target] if isinstance(x, DeviceArray)), current_device())
    descending = False
    if not isinstance(sp, DeviceArray) and sp.size:  # the reference's ordering decision on the first column (monotonic.py:84-89)
        s0 = np.asarray(sp, dtype=dtype).reshape(-1)[:1]
        a, b = A.astype(dtype), B.astype(dtype)
        ph = a[[0, 1, -2, -1]] + b[[0, 1, -2, -1]] * s0
        pf = ph[[0, 2]] + 0.5 * (ph[[1, 3]] - ph[[0, 2]])
        descending = not bool(pf[0] < pf[1])
    out = _interp_run(data, target, interpolation, aux, descending, dtype, out_dtype, device, cols, hybrid=(A, B, sp))
    return _interp_finish(out, on_device, out_dtype, vertical_axis)


@_foreign_aware("data", "target_h", "t", "q", "zs", "sp", "aux_bottom_data", "aux_bottom_h", "aux_top_data", "aux_top_h")
def interpolate_hybrid_to_height_levels(data, target_h, t, q, zs, A, B, sp, alpha_top="ifs", h_type="geometric",
                                        h_reference="ground", interpolation="linear", aux_bottom_data=None,
                                        aux_bottom_h=None, aux_top_data=None, aux_top_h=None, vertical_axis=0):
    """Interpolate `data` from hybrid full levels to height levels (vertical.py:1329-1486): `height_on_hybrid_levels`
    (one column scan) writing a device-resident height field that feeds the kernel of `interpolate_monotonic`; the
    height field is never copied to the host, for NumPy input either."""
    if interpolation not in _INTERP_MODE:
        raise ValueError(f"Unknown interpolation method '{interpolation}'. Supported methods are 'linear', 'log' and 'nearest'.")
    if h_reference not in ["sea", "ground"]:
        raise ValueError(f"Unknown '{h_reference=}'. Use 'sea' or 'ground'.")
    others = (data, target_h, t, q, zs, sp, aux_bottom_data, aux_bottom_h, aux_top_data, aux_top_h)
    on_device = any(isinstance(x, DeviceArray) for x in others)
    if on_device and vertical_axis != 0:
        raise ValueError("DeviceArray input: fields are level-major, vertical_axis must be 0")
    key = ("geometric" if h_type == "geometric" else "geopotential", h_reference)
    h = _chain(t, q, zs, A, B, sp, alpha_top, _GEO_MODE[key], vertical_axis, device_result=True)
    # aux_bottom_* lies at the smallest height (aux_min_level_*), aux_top_* at the largest (vertical.py:1476-1486)
    return _monotonic(data, h, target_h, interpolation, aux_bottom_data, aux_bottom_h, aux_top_data, aux_top_h, vertical_axis,
                      on_device=on_device)


@_foreign_aware("data", "target_h", "z", "zs", "aux_bottom_data", "aux_bottom_h", "aux_top_data", "aux_top_h")
def interpolate_pressure_to_height_levels(data, target_h, z, zs, h_type="geometric", h_reference="ground",
                                          interpolation="linear", aux_bottom_data=None, aux_bottom_h=None, aux_top_data=None,
                                          aux_top_h=None, vertical_axis=0):
    """Interpolate `data` from pressure levels to height levels (vertical.py:1489-1613): the height of the levels is
    formed from the geopotential `z` (and `zs` for heights above ground) by one elementwise kernel into a device-resident
    temporary, which feeds `interpolate_monotonic`.  As in the reference, any `h_type` but "geometric" means
    geopotential height and any `h_reference` but "ground" means above sea level."""
    if interpolation not in _INTERP_MODE:
        raise ValueError(f"Unknown interpolation method '{interpolation}'. Supported methods are 'linear', 'log' and 'nearest'.")
    z, zs_in = _host_or_dev(z), _host_or_dev(zs)
    others = [_host_or_dev(x) for x in (data, target_h, aux_bottom_data, aux_bottom_h, aux_top_data, aux_top_h)]
    on_device = any(isinstance(x, DeviceArray) for x in [z, zs_in] + others)
    if on_device and vertical_axis != 0:
        raise ValueError("DeviceArray input: fields are level-major, vertical_axis must be 0")
    if not isinstance(z, DeviceArray) and vertical_axis != 0 and z.ndim > 1:
        z = np.moveaxis(z, vertical_axis, 0)
    if len(z.shape) == 0:
        raise ValueError("At least two levels are required for interpolation.")
    ground = h_reference == "ground"
    mode = (4 if ground else 2) if h_type == "geometric" else (5 if ground else 3)
    cols = tuple(z.shape[1:])
    parts = [z.dtype] + ([zs_in.dtype] if ground else [])
    dtype = _arith_dtype(parts) if all(np.dtype(p).kind == "f" for p in parts) else _F64
    device = next((x.device for x in [z, zs_in] + others if isinstance(x, DeviceArray)), current_device())
    stream = current_stream()
    d_z = _to_device(z, dtype, device)
    d_zs = None
    if ground:
        if isinstance(zs_in, DeviceArray) and tuple(zs_in.shape) != cols and not (zs_in.size == 1 and math.prod(cols) == 1):
            raise ValueError(f"zs {tuple(zs_in.shape)} does not match a level of z {cols}")
        d_zs = _to_device(zs_in, dtype, device, None if isinstance(zs_in, DeviceArray) else cols)
        d_zs.on(stream)
    h = DeviceArray.empty(tuple(z.shape), dtype, device)
    tag = "f32" if dtype == _F32 else "f64"
    _ffi.check(getattr(_ffi.lib(), f"ekm_height_from_geopotential_{tag}")(
        device, stream, d_z.on(stream), d_zs.ptr if d_zs is not None else None, int(math.prod(cols)), int(z.shape[0]), mode,
        h.on(stream)))
    # aux_bottom_* lies at the smallest height (aux_min_level_*), aux_top_* at the largest (vertical.py:1603-1613)
    return _monotonic(data, h, target_h, interpolation, aux_bottom_data, aux_bottom_h, aux_top_data, aux_top_h, vertical_axis,
                      on_device=on_device)


_LEVEL_TABLES = None


def hybrid_level_parameters(n_levels, model="ifs"):
    """The A and B half-level coefficients of a hybrid-level configuration (vertical/array/hybrid.py:40-102):
    two float64 arrays of length n_levels + 1; `model="ifs"` with 91 or 137 levels, same errors as the
    reference.  The tables are the constant data of the reference's conf/ifs_levels_conf.json, recorded into
    ekm_hip/data/ifs_levels.npz by tests/golden/gen_golden_vertical.py and shipped inside the package."""
    global _LEVEL_TABLES
    import os

    if _LEVEL_TABLES is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "ifs_levels.npz")
        with np.load(path) as f:
            tabs = {}
            for key in f.files:
                mdl, n, which = key.split(".")
                tabs.setdefault(mdl, {}).setdefault(n, {})[which] = f[key]
        _LEVEL_TABLES = tabs
    model = model.lower()
    n_levels = str(n_levels)
    if model in _LEVEL_TABLES:
        if n_levels in _LEVEL_TABLES[model]:
            c = _LEVEL_TABLES[model][n_levels]
            return c["A"], c["B"]
        raise ValueError(f"Hybrid level parameters not available for {n_levels} levels in model '{model}'.")
    raise ValueError(f"Model '{model}' not recognized for hybrid level parameters.")


class HybridPressure:
    """Pressure on hybrid full levels given by its definition, p_k(x) = p_half[k] + 0.5*(p_half[k+1]-p_half[k])
    with p_half[h] = A[h] + B[h]*sp(x), for use in place of a pressure field in ekm_hip.thermo calls on
    `[level, ...sp.shape]` fields: the kernels form p from `sp` and the LDS-resident A/B tables, so the
    pressure field is never read from (or written to) HBM."""

    def __init__(self, A, B, sp):
        self.A = np.array(A, dtype=np.float64, order="C")  # copies: the device tables made from them are kept (device_tables)
        self.B = np.array(B, dtype=np.float64, order="C")
        if self.A.ndim != 1 or self.A.shape != self.B.shape or self.A.size < 2:
            raise ValueError("A and B must be 1-D half-level tables of the same length >= 2")
        self.sp = sp
        self.nlev = self.A.size - 1
        # leading pure pressure levels (B = 0 on both half levels: the upper 53 of the 137 IFS levels): the library runs
        # them at level-vector speed in a launch of their own (ekm_operand.nflat)
        nz = np.flatnonzero(self.B != 0.0)
        self.nflat = int(max(0, (nz[0] if nz.size else self.B.size) - 1))
        self._tables = {}  # (device, dtype) -> the two tables in device memory, uploaded once

    def device_tables(self, device, dtype):
        """A and B in `dtype` on `device`, uploaded at the first use there (synchronously: any stream may read them
        afterwards) and kept with this object.  Inside an `ekm_hip.graph()` block nothing can be uploaded: use the object
        once, or call this, before the block."""
        key = (int(device), np.dtype(dtype).char)
        tabs = self._tables.get(key)
        if tabs is None:
            tabs = self._tables[key] = tuple(DeviceArray.from_host(x.astype(dtype), device=device) for x in (self.A, self.B))
        return tabs

    @property
    def shape(self):
        return (self.nlev,) + tuple(np.shape(self.sp))


# `earthkit.meteo.vertical.array.<name>` is how the reference reaches the array-level functions
# (vertical/__init__.py:20, vertical/array/__init__.py:14-15): same module here.
import sys as _sys  # noqa: E402

array = _sys.modules[__name__]
