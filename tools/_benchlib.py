"""What the per-family benchmark tools (tools/bench_*.py) share: how they open the device, time, and write.

How every GPU timing is taken: HIP events on the null stream around `steps` launches after `warmup` launches, in ONE
process on the same arrays; the time is the events' elapsed time over `steps`.  `EventTimer.mean` is that one figure;
`EventTimer.repeated` warms up once and takes the window `reps` times (the caller reports median / min / max).  The
copy beside a kernel time is ekm_stream_mix (`nin` streams in, `nout` out, no arithmetic) timed the same way.

Importing this module loads no library and opens no device: `open_device` does.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "earthkit-meteo_amd"))

HBM_PEAK = 8.0e12


def parser(out_name):
    """The flags every tool has; `--out` defaults to profiles/<out_name>."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    return ap


def open_device(dev=0):
    """Loads the library and initialises it: (lib, dev, device name)."""
    from ekm_hip import _ffi

    lib = _ffi.lib()
    _ffi.check(lib.ekm_init())
    name = C.create_string_buffer(128)
    lib.ekm_device_name(dev, name, 128)
    return lib, dev, name.value.decode()


def tag(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def whole_words(nbytes):
    """ekm_stream_mix copies whole 16-byte words: the bytes it moves of `nbytes`."""
    return nbytes - nbytes % 16


class EventTimer:
    """Two events, created here and destroyed when the `with` block ends."""

    def __init__(self, lib, dev, steps, warmup):
        from ekm_hip import _ffi

        self.lib, self.dev, self.steps, self.warmup, self.check = lib, dev, steps, warmup, _ffi.check
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            self.check(lib.ekm_event_create(dev, C.byref(e)))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        rcs = [self.lib.ekm_event_destroy(self.dev, e) for e in self.ev]
        if exc_type is None:  # (an error on the way out of a failed run would hide the failure)
            for rc in rcs:
                self.check(rc)

    def _window(self, launch):
        lib, dev, ev = self.lib, self.dev, self.ev
        self.check(lib.ekm_event_record(dev, ev[0], None))
        for _ in range(self.steps):
            launch()
        self.check(lib.ekm_event_record(dev, ev[1], None))
        self.check(lib.ekm_event_sync(dev, ev[1]))
        ms = C.c_float()
        self.check(lib.ekm_event_elapsed_ms(dev, ev[0], ev[1], C.byref(ms)))
        return ms.value / self.steps

    def mean(self, launch):
        """ms per launch."""
        for _ in range(self.warmup):
            launch()
        return self._window(launch)

    def repeated(self, launch, reps):
        """ms per launch of `reps` windows after one warm-up."""
        for _ in range(self.warmup):
            launch()
        return [self._window(launch) for _ in range(reps)]

    def copy(self, srcs, dsts, nbytes, reps=None):
        """ms of one ekm_stream_mix of `whole_words(nbytes)` from every pointer of `srcs` to every pointer of `dsts`
        (`mean`, or `repeated` where `reps` is given)."""
        ins, outs = (C.c_void_p * len(srcs))(*srcs), (C.c_void_p * len(dsts))(*dsts)
        nbytes = whole_words(nbytes)
        launch = lambda: self.check(self.lib.ekm_stream_mix(self.dev, None, ins, len(srcs), outs, len(dsts), nbytes))  # noqa: E731
        return self.mean(launch) if reps is None else self.repeated(launch, reps)


def derived(ms, nbytes, copy_rate, points=None):
    """The standard fields of a run of `ms` over `nbytes` algorithmic bytes beside a copy at `copy_rate` bytes/s;
    `copy_ms_same_bytes` is the time that rate needs for `nbytes`.  A tool writes the ones its file has."""
    rate = nbytes / (ms * 1e-3)
    out = dict(bytes_per_s=rate)
    if copy_rate is not None:
        out.update(copy_bytes_per_s=copy_rate, copy_ms_same_bytes=nbytes / copy_rate * 1e3, frac_copy_rate=rate / copy_rate)
    out["frac_hbm_peak"] = rate / HBM_PEAK
    if points is not None:
        out["points_per_s"] = points / (ms * 1e-3)
    return out


def tiled_rows(base, npts, dtype):
    """[rows, npts] on the device: the distinct columns of `base` [rows, distinct] tiled over the field, row by row."""
    import ekm_hip

    rows, reps = base.shape[0], (npts + base.shape[1] - 1) // base.shape[1]
    d = ekm_hip.DeviceArray.empty((rows, npts), dtype)
    for k in range(rows):
        d.flat_slice(k * npts, (k + 1) * npts).copy_from_host(np.tile(base[k], reps)[:npts].astype(dtype))
    return d


def one_level_long_quantiles(lib, dev, sample, m, npts, out):
    """A launch of ekm_long_quantiles_* for the median of `sample` [m, npts] (sample axis first): the tile load and sort of
    the long-axis kernels with the cheapest read-out there is.  Returns (launch, the tables to keep alive)."""
    import ekm_hip
    from ekm_hip import _ffi, stats

    dt = np.dtype(sample.dtype)
    tabs = [ekm_hip.DeviceArray.from_host(np.ascontiguousarray(t)) for t in stats.quantile_positions("numpy", m, [0.5], dt)]
    fn = getattr(lib, "ekm_long_quantiles_" + tag(dt))
    return (lambda: _ffi.check(fn(dev, None, sample.ptr, 1, m, npts, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, 1, _ffi.QUANTILE_LERP,
                                  out.ptr))), tabs


def merge(path, result):
    """`write`, keeping the keys another tool wrote into the same file."""
    if os.path.exists(path):
        with open(path) as f:
            result = {**json.load(f), **result}
    write(path, result)


def emit(result, key, run):
    """Appends the run to its list in `result` and prints it as one JSON line."""
    result[key].append(run)
    print(json.dumps(run), flush=True)


def write(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
