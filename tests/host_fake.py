"""A fake device for the Python host layer: the volume-op methods of host.Device run on it without the library or a GPU.

Device memory is a set of numbered bytearrays behind fake addresses; the library is a stub whose every svr_* function appends one record
to a transcript -- the function's name and its arguments rendered without addresses -- and returns 0.  The stub can fail the k-th
library call or the k-th malloc, so a test sees what a method leaves allocated on every way out.  tests/test_host_staging_cpu.py replays
the rows of tests/golden/make_host_call_transcript.py on it."""
import ctypes as C
import hashlib

import numpy as np

from sunvolumerender_amd import abi
from sunvolumerender_amd.host import SvrError
from sunvolumerender_amd.volume_ops import VolumeOps

FAKE_BASE = 1 << 60            # fake device addresses: FAKE_BASE + (allocation number << 32) + offset; host addresses lie far below
MESH_COUNTS = (4, 2)           # the vertices and triangles that the counting call of svr_mesh_isosurface / _region reports


def _sha1(data) -> str:
    return hashlib.sha1(bytes(data)).hexdigest()


class Dev:
    """Row argument: the array in a device buffer of the caller (a bool mask as its bit mask); the method gets the pointer."""

    def __init__(self, array):
        self.array = array


class Out:
    """Row argument: a zeroed device buffer of the caller of nbytes bytes, for out_ptr= and its kin."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)


class Lib:
    """Row argument: the stub library itself, for the module-level functions that take lib."""


class StubLib:
    VALUES = {"svr_histogram_bins": lambda p: ((p.hi - p.lo) >> p.shift) + 1}      # functions whose return value is no status

    def __init__(self, dev):
        self.dev = dev
        self.calls, self.syncs, self.last_sync_at = [], 0, -1
        self.fail_call, self.ncalls, self.err = None, 0, (0, b"")

    def __getattr__(self, name):
        if not name.startswith("svr_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, *args)

    def _call(self, name, *args):
        if name == "svr_device_synchronize":
            self.syncs, self.last_sync_at = self.syncs + 1, len(self.calls)
            return 0
        if name == "svr_last_error_code":
            return self.err[0]
        if name == "svr_last_error":
            return self.err[1]
        if name == "svr_clear_error":
            self.err = (0, b"")
            return 0
        self.calls.append({"fn": name, "args": [self.dev.render(a) for a in args]})
        if name in self.VALUES:
            return self.VALUES[name](args[0]._obj)
        self.ncalls += 1
        if self.ncalls == self.fail_call:
            self.err = (-1, b"injected failure of " + name.encode())
            return -1
        if name in ("svr_mesh_isosurface", "svr_mesh_region"):
            info = args[-1]._obj
            if not info.vertices:
                info.vertices, info.triangles = MESH_COUNTS
        return 0


class FakeDevice(VolumeOps):
    def __init__(self):
        self.mem, self.next, self.host = {}, 1, {}
        self.nmalloc, self.fail_malloc = 0, None
        self.lib = StubLib(self)

    # ---- what the volume ops need of a Device ----
    def check(self, rc=0):
        code = self.lib.svr_last_error_code()
        if rc != 0 or code != 0:
            msg = self.lib.svr_last_error().decode()
            self.lib.svr_clear_error()
            raise SvrError(f"libsvr_hip error {code}: {msg}")

    def synchronize(self):
        self.check(self.lib.svr_device_synchronize())

    def malloc(self, nbytes: int) -> int:
        self.nmalloc += 1
        if self.nmalloc == self.fail_malloc:
            raise SvrError("injected malloc failure")
        assert int(nbytes) > 0, "malloc of no bytes"
        ptr = FAKE_BASE + (self.next << 32)
        self.mem[ptr], self.next = bytearray(int(nbytes)), self.next + 1
        return ptr

    def free(self, ptr: int):
        assert ptr in self.mem, f"free of {ptr:#x}: freed before, or never allocated"
        del self.mem[ptr]

    def _span(self, ptr, nbytes=None):
        base, off = ptr & ~0xFFFFFFFF, ptr & 0xFFFFFFFF
        assert base in self.mem, f"{ptr:#x} is no live device pointer"
        buf = self.mem[base]
        nbytes = len(buf) - off if nbytes is None else nbytes
        assert 0 <= off and off + nbytes <= len(buf), f"{nbytes} bytes at offset {off} of a buffer of {len(buf)}"
        return buf, off, nbytes

    def to_device(self, ptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        buf, off, n = self._span(ptr, arr.nbytes)
        buf[off:off + n] = arr.tobytes()

    def to_host(self, ptr: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        buf, off, n = self._span(ptr, out.nbytes)
        return np.frombuffer(bytes(buf[off:off + n]), dtype=dtype).reshape(out.shape).copy()

    @property
    def live(self):
        return set(self.mem)

    # ---- rendering of arguments and results without addresses ----
    def know(self, array):
        """A host array whose address may reach the library: it is rendered with its contents."""
        self.host[array.ctypes.data] = array

    def _pointer(self, v):
        if not v:
            return None
        if v >= FAKE_BASE:
            buf, off, n = self._span(v)
            return ["dev", n, _sha1(buf[off:])] + ([off] if off else [])
        a = self.host.get(v)
        return ["host"] if a is None else ["host", a.nbytes, _sha1(a.tobytes())]

    def render(self, x):
        if x is None or isinstance(x, (bool, int, float, str)):
            return self._pointer(x) if isinstance(x, int) and not isinstance(x, bool) and x >= FAKE_BASE else x
        if isinstance(x, (tuple, list)):
            return [self.render(t) for t in x]
        if isinstance(x, np.ndarray):
            return ["array", x.dtype.str if x.dtype.names is None else str(x.dtype.itemsize), list(x.shape), _sha1(np.ascontiguousarray(x).tobytes())]
        if isinstance(x, np.generic):
            return x.item()
        if hasattr(x, "_obj"):                                # byref(...)
            return self.render(x._obj)
        if isinstance(x, C.c_void_p):
            return self._pointer(x.value)
        if isinstance(x, C._Pointer):
            return self._pointer(C.cast(x, C.c_void_p).value)
        if isinstance(x, C.Structure):
            return {name: self._member(getattr(x, name), ftype) for name, ftype, *_ in x._fields_}
        if isinstance(x, C.Array):
            return [self._member(t, x._type_) for t in x]
        if isinstance(x, C._SimpleCData):
            return x.value
        raise TypeError(f"cannot render {type(x)}")

    def _member(self, v, ftype):
        if ftype is C.c_void_p:
            return self._pointer(v)
        if issubclass(ftype, C._Pointer):
            return self._pointer(C.cast(v, C.c_void_p).value)
        return self.render(v)


def pack(array):
    """What a caller uploads for a row argument: the bit mask of a bool array, any other array as it is."""
    from sunvolumerender_amd import host
    return host.region_mask_pack(array) if array.dtype == bool else np.ascontiguousarray(array)


def run_row(row, dev=None, fail_call=None, fail_malloc=None):
    """Runs one row (id, callable name, args, kwargs) on a fresh FakeDevice: Dev / Out arguments become buffers of the caller, host arrays
    are made known to the stub.  Returns (dev, caller buffers, result or the exception raised)."""
    from sunvolumerender_amd import host
    _, name, args, kwargs = row
    dev = dev if dev is not None else FakeDevice()
    caller = []

    def resolve(a):
        if isinstance(a, Dev):
            data = pack(a.array)
            caller.append(dev.malloc(max(data.nbytes, 4)))
            dev.to_device(caller[-1], data)
            return caller[-1]
        if isinstance(a, Out):
            caller.append(dev.malloc(a.nbytes))
            return caller[-1]
        if isinstance(a, Lib) or a is Lib:
            return dev.lib
        if isinstance(a, np.ndarray):
            dev.know(a)
        return a
    args, kwargs = [resolve(a) for a in args], {k: resolve(v) for k, v in kwargs.items()}
    dev.nmalloc, dev.fail_malloc, dev.lib.fail_call = 0, fail_malloc, fail_call
    fn = getattr(host, name[5:]) if name.startswith("host.") else getattr(dev, name)
    try:
        result = fn(*args, **kwargs)
    except Exception as e:                                    # the caller looks at it
        result = e
    return dev, caller, result
