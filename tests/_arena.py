"""A guarded arena: the inputs and outputs of ONE kernel call laid out inside one device allocation, so that what the
kernel did OUTSIDE the elements it was asked for can be inspected afterwards.

The parity tests read back exactly `n` elements of buffers the Python layer allocated; a store a few elements past the
end of an output, in front of it, or into an input goes unseen there (GPU AddressSanitizer is not an option on shared
machines).  Here
  * every buffer has GUARD_BYTES of a fixed 32-bit pattern in front of it and behind it.  256 KiB = 16 tiles x 1024
    lanes x 16 B: as far as ONE mis-indexed workgroup of the largest launch shape in csrc/map_kernel.hpp can reach, so
    a stray store of that kind lands in memory this process owns;
  * outputs are pre-filled with UNWRITTEN, a NaN (in fp32, and in both halves of an fp64) whose payload no input of
    these tests carries and no arithmetic produces (a generated NaN is the default 0x7fc00000 / 0x7ff8000000000000, a
    propagated one carries an input's payload): "never written" can be told from "computed NaN";
  * a buffer starts 16-B aligned, or `offset` elements behind a 16-B boundary;
  * `check()` downloads the arena once and raises ArenaError naming the buffer, the element index and the pattern found
    if a guard word changed, an input differs from what was uploaded, or an output element still holds UNWRITTEN.

The memory behind it is a backend: DeviceMemory (libekm_thermo.so: ekm_malloc / ekm_fill_u32 / ekm_h2d / ekm_d2h), or
HostMemory -- a NumPy array standing in for the device, so that this judge has negative tests of its own in the CPU
suite (tests/test_arena.py).
"""
import ctypes as C

import numpy as np

GUARD_BYTES = 256 * 1024
GUARD_WORD = 0xA5C35A3C       # a tiny negative number in fp32 and (both words) in fp64: nothing a thermo kernel returns
UNWRITTEN = 0x7FF8A17E        # fp32: a quiet NaN with payload 0x78a17e; twice: an fp64 quiet NaN with payload 0x8a17e7ff8a17e
_U32 = np.dtype(np.uint32)
_KIND = {"in": "input", "out": "output", "inout": "in-out buffer"}


class ArenaError(AssertionError):
    pass


class HostMemory:
    """A NumPy array in place of device memory; "pointers" are byte offsets into `mem`."""

    def alloc(self, nbytes):
        self.mem = np.zeros(nbytes, np.uint8)
        return 0

    def fill_u32(self, ptr, word, count):
        self.mem[ptr:ptr + 4 * count].view(_U32)[:] = word

    def upload(self, ptr, host):
        self.mem[ptr:ptr + host.nbytes] = host.reshape(-1).view(np.uint8)

    def download(self, ptr, nbytes):
        return self.mem[ptr:ptr + nbytes].copy()

    def view(self, ptr, dtype, count):
        """(fake kernels write through this)"""
        return self.mem[ptr:ptr + count * np.dtype(dtype).itemsize].view(dtype)

    def free(self):
        self.mem = None


class DeviceMemory:
    """One ekm_malloc block on `device`; fills and copies are queued on `stream`, `download` waits for them."""

    def __init__(self, device=0, stream=None):
        from ekm_hip import _ffi

        self._ffi, self.lib, self.device, self.stream, self.base = _ffi, _ffi.lib(), device, stream, None

    def alloc(self, nbytes):
        out = C.c_void_p()
        self._ffi.check(self.lib.ekm_malloc(self.device, nbytes, C.byref(out)))
        self.base = out.value
        return self.base

    def fill_u32(self, ptr, word, count):
        self._ffi.check(self.lib.ekm_fill_u32(self.device, ptr, word, count, self.stream))

    def upload(self, ptr, host):
        self._ffi.check(self.lib.ekm_h2d(self.device, ptr, host.ctypes.data, host.nbytes, self.stream))
        self._ffi.check(self.lib.ekm_stream_sync(self.device, self.stream))  # `host` may go away

    def download(self, ptr, nbytes):
        out = np.empty(nbytes, np.uint8)
        self._ffi.check(self.lib.ekm_d2h(self.device, out.ctypes.data, ptr, nbytes, self.stream))
        self._ffi.check(self.lib.ekm_stream_sync(self.device, self.stream))
        return out

    def free(self):
        if self.base:
            self._ffi.check(self.lib.ekm_stream_sync(self.device, self.stream))
            self._ffi.check(self.lib.ekm_free(self.device, self.base))
            self.base = None


class _Buffer:
    __slots__ = ("name", "kind", "dtype", "count", "start", "host")


class Arena:
    """arena = Arena(memory); arena.input("t", array, offset=1); arena.output("out", n, np.float32); arena.commit();
    launch on arena.ptr(name); arena.check(); arena.result("out").

    `input`: uploaded, must come back bit for bit.  `output`: pre-filled with UNWRITTEN, every element must have been
    written.  `inout(name, array)`: uploaded, guarded, contents not judged (a flag word the kernel ORs into)."""

    def __init__(self, memory):
        self.mem, self.bufs, self.size, self.base, self.image = memory, {}, GUARD_BYTES, None, None

    def _add(self, name, kind, dtype, count, offset, host):
        assert self.base is None and name not in self.bufs and count >= 0
        b = _Buffer()
        b.name, b.kind, b.dtype, b.count, b.host = name, kind, np.dtype(dtype), int(count), host
        assert b.dtype.itemsize in (4, 8)
        b.start = (self.size + 15) // 16 * 16 + int(offset) * b.dtype.itemsize
        self.size = (b.start + b.count * b.dtype.itemsize + 3) // 4 * 4 + GUARD_BYTES
        self.bufs[name] = b
        return b

    def input(self, name, array, offset=0):
        a = np.ascontiguousarray(array).reshape(-1)
        return self._add(name, "in", a.dtype, a.size, offset, a.copy())

    def inout(self, name, array, offset=0):
        a = np.ascontiguousarray(array).reshape(-1)
        return self._add(name, "inout", a.dtype, a.size, offset, a.copy())

    def output(self, name, count, dtype, offset=0):
        return self._add(name, "out", dtype, count, offset, None)

    def commit(self):
        self.size = (self.size + 15) // 16 * 16
        self.base = self.mem.alloc(self.size)
        self.mem.fill_u32(self.base, GUARD_WORD, self.size // 4)
        for b in self.bufs.values():
            if b.kind == "out":
                if b.count:
                    self.mem.fill_u32(self.base + b.start, UNWRITTEN, b.count * b.dtype.itemsize // 4)
            elif b.count:
                self.mem.upload(self.base + b.start, b.host)
        return self

    def ptr(self, name):
        return self.base + self.bufs[name].start

    def check(self):
        """Downloads the arena (once; `result` reads from this image) and judges it."""
        self.image = img = self.mem.download(self.base, self.size)
        words = img.view(_U32)
        guard = np.ones(words.size, bool)
        for b in self.bufs.values():
            guard[b.start // 4:(b.start + b.count * b.dtype.itemsize) // 4] = False
        bad = np.flatnonzero(guard & (words != GUARD_WORD))
        if bad.size:
            w = int(bad[0])
            # the buffer the word is nearest to, and where it lies in that buffer's element numbering
            def dist(b):
                lo, hi = b.start // 4, (b.start + b.count * b.dtype.itemsize) // 4
                return lo - w if w < lo else w - hi + 1
            b = min(self.bufs.values(), key=dist)
            elem = (w * 4 - b.start) // b.dtype.itemsize  # floor: negative in front of the buffer, >= count behind it
            where = "before the start of" if elem < 0 else "past the end of"
            raise ArenaError(f"guard word changed {where} {_KIND[b.kind]} '{b.name}' ({b.count} elements): element index {elem}, "
                             f"found 0x{int(words[w]):08x}; {bad.size} guard words changed in all")
        for b in self.bufs.values():
            raw = img[b.start:b.start + b.count * b.dtype.itemsize]
            if b.kind == "in":
                diff = np.flatnonzero(raw.view(b.dtype).view(f"u{b.dtype.itemsize}") != b.host.view(f"u{b.dtype.itemsize}"))
                if diff.size:
                    i = int(diff[0])
                    raise ArenaError(f"input '{b.name}' was modified: element index {i} holds 0x{int(raw.view(f'u{b.dtype.itemsize}')[i]):x}, "
                                     f"uploaded 0x{int(b.host.view(f'u{b.dtype.itemsize}')[i]):x}; {diff.size} elements differ")
            elif b.kind == "out":
                w = raw.view(_U32).reshape(b.count, b.dtype.itemsize // 4)
                left = np.flatnonzero((w == UNWRITTEN).all(axis=1))
                if left.size:
                    raise ArenaError(f"output '{b.name}' ({b.count} elements): element index {int(left[0])} was never written (still holds "
                                     f"0x{UNWRITTEN:08x}); {left.size} elements unwritten, the last at index {int(left[-1])}")

    def result(self, name):
        b = self.bufs[name]
        assert self.image is not None, "check() first"
        return self.image[b.start:b.start + b.count * b.dtype.itemsize].view(b.dtype).copy()

    def free(self):
        self.mem.free()
