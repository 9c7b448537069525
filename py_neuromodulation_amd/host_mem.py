"""Host memory around the engine: the conversion threads, the recycled result tables, the page-locked staging pools and
the staging thread of a pipelined batch.  Needs the library only where it is handed one."""

from __future__ import annotations

import atexit
import collections
import ctypes as C
import functools
import os
import threading

import numpy as np

from . import _lib


@functools.lru_cache(None)
def _pool():
    """A few host threads for the dtype conversions around a batch (NumPy's casting loops release the GIL):
    float64 recording -> float32 staging and float32 features -> float64 table are 100+ MB each.  (Built on first use.)"""
    from concurrent.futures import ThreadPoolExecutor

    return ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) // 2)))


def _rows_ok(a: np.ndarray, *dtypes) -> bool:
    """libnmx can read these rows in place: 2-D, one of ``dtypes``, unit stride along a row, a whole positive row pitch."""
    return (a.ndim == 2 and a.dtype in dtypes and a.strides[1] == a.itemsize and a.strides[0] > 0
            and a.strides[0] % a.itemsize == 0)


def _ld(a: np.ndarray) -> int:
    """Row pitch of a row-contiguous 2-D array in elements.  (NumPy is free to report ANY stride along an axis of
    length one -- the transpose of a (samples, 1) array has a row "pitch" of one element: a single row's pitch is its
    length.)"""
    return a.strides[0] // a.itemsize if a.shape[0] > 1 else max(a.shape[1], 1)


def parallel_cast(dst: np.ndarray, src: np.ndarray, sub: np.ndarray | None = None, lib=None) -> None:
    """dst[...] = src (with cast), first axis split over the conversion threads.  ``sub``: one float64 constant per row,
    subtracted BEFORE the cast (the engine's offset split: the cast then rounds at the signal's magnitude).  With the
    loaded library and row-contiguous float arrays the pass runs in libnmx's staging helpers (nmx_host_stage_rows /
    nmx_host_widen_rows: one pass at memory speed; NumPy's buffered casts manage 1 - 3 GB/s) -- same values."""
    n = dst.shape[0]
    if lib is not None and dst.ndim == 2 and dst.shape == getattr(src, "shape", None) and dst.size:
        if _rows_ok(dst, np.float32) and _rows_ok(src, np.float32, np.float64):
            k = None if sub is None else np.ascontiguousarray(sub, dtype=np.float64)
            lib.check(lib.lib.nmx_host_stage_rows(dst.ctypes.data, dst.strides[0] // 4, src.ctypes.data,
                                                  int(src.dtype == np.float64), src.strides[0] // src.itemsize, None, n, 0,
                                                  dst.shape[1], None if k is None else k.ctypes.data, 0))
            return
        if sub is None and _rows_ok(dst, np.float64) and _rows_ok(src, np.float32):
            runs = np.array([0, 0, dst.shape[1]], dtype=np.int64)
            lib.check(lib.lib.nmx_host_widen_rows(dst.ctypes.data, dst.strides[0] // 8, src.ctypes.data, src.strides[0] // 4,
                                                  0, n, runs.ctypes.data, 1, 0))
            return

    def put(a, b):
        if sub is None:
            dst[a:b] = src[a:b]
        else:
            dst[a:b] = np.asarray(src[a:b], dtype=np.float64) - sub[a:b, None]

    if dst.size < (1 << 20) or n < 2:
        put(0, n)
        return
    k = min(n, 8)
    edges = [(i * n) // k for i in range(k + 1)]
    list(_pool().map(lambda i: put(edges[i], edges[i + 1]), range(k)))


class _TableLease:
    """Owner of a result table's memory: hands its buffer back to the pool when the last array on it is gone."""

    def __init__(self, raw: np.ndarray, pool: "_TablePool") -> None:
        self._raw, self._pool = raw, pool
        self.__array_interface__ = raw.__array_interface__

    def __del__(self):
        try:
            self._pool._give_back(self._raw)
        except Exception:   # (interpreter shutdown)
            pass


class _TablePool:
    """Recycled float64 result tables.  A stream of the reference's shape hands a fresh [hops, features] float64 table to
    its caller per run (stream/stream.py:319-343): 75 - 80 MB whose first touch is ~20 000 page faults and whose release
    another ~3 ms of munmap (measured on the GPU box: touch 4 - 85 ms depending on what the kernel finds for its huge
    pages, free 2.8 - 3.2 ms), per run, on the caller's thread.  The tables here are ordinary ndarrays whose memory goes
    back to this pool instead of the system when the caller drops them (DataFrame included) -- the next run finds its pages
    mapped.  At most ``keep`` idle buffers are held (``release_tables()`` frees them); small tables are not pooled."""

    MIN_BYTES = 1 << 22

    def __init__(self, keep: int = 2) -> None:
        self.keep, self._free, self._lock = keep, [], threading.Lock()
        # buffers coming home from `_TableLease.__del__`: a finaliser can run on ANY allocation of the thread that holds
        # the lock (a cyclic-GC pass inside `empty`), so it takes no lock -- deque.append is atomic -- and the list is
        # merged by the next call that does
        self._returned = collections.deque()

    def _merge(self) -> None:   # (lock held)
        while self._returned:
            self._free.append(self._returned.popleft())
        del self._free[:max(0, len(self._free) - self.keep)]

    def empty(self, shape, fill=None) -> np.ndarray:
        n = int(np.prod(shape))
        if n * 8 < self.MIN_BYTES:
            return np.empty(shape) if fill is None else np.full(shape, fill)
        raw = None
        with self._lock:
            self._merge()
            for i in range(len(self._free)):
                if n <= self._free[i].size <= n + n // 4:
                    raw = self._free.pop(i)
                    break
        if raw is None:
            raw = np.empty(n)
        arr = np.asarray(_TableLease(raw, self))[:n].reshape(shape)
        if fill is not None:
            arr.fill(fill)
        return arr

    def _give_back(self, raw: np.ndarray) -> None:
        self._returned.append(raw)
        if len(self._returned) > 2 * self.keep + 2 and self._lock.acquire(blocking=False):   # (nobody allocates: trim here)
            try:
                self._merge()
            finally:
                self._lock.release()

    def clear(self) -> int:
        with self._lock:
            self._merge()
            n = len(self._free)
            self._free.clear()
        return n


_TABLES = _TablePool()


def table_empty(shape, fill=None) -> np.ndarray:
    """A float64 result table from the recycling pool (``_TablePool``)."""
    return _TABLES.empty(shape, fill)


def release_tables() -> int:
    """Free the idle result-table buffers of the pool; returns how many."""
    return _TABLES.clear()


_STAGING: dict = {}


def _staging(lib, device: int = 0, slot: int = 0) -> "_Pinned":
    """ONE staging pool per loaded library, shared by every engine (page-locking ~170 MB costs tens of
    milliseconds -- Stream.run builds a fresh engine per run, like the reference builds a fresh
    DataProcessor).  Engines are not re-entrant (include/nmx.h), neither is the pool -- one pool per device AND
    ``slot``: the engines of a multi-device stream run on one host thread each and take the slot of their part index,
    so two parts never share a staging array even when they name the same device (``devices=[0, 0]``).  Pools are
    reference counted (``users``: an engine that closes gives its count back) and stay cached: page-locking ~170 MB again
    costs ~17 ms per Stream (measured: 8 ms hipHostMalloc + 9 ms hipHostFree against a 29 ms Stream.run), and the size is
    bounded by the largest batch ever staged (two named arrays, grown on demand).  ``release_staging()`` frees the pools
    nobody uses; every pool is freed at interpreter exit."""
    key = (str(lib.path), int(device), int(slot))
    if key not in _STAGING:
        _STAGING[key] = _Pinned(lib, key)
    _STAGING[key].users += 1
    return _STAGING[key]


def release_staging() -> int:
    """Free the page-locked staging pools that no open engine uses -- and hand the device memory libnmx keeps of destroyed
    plans back to the driver (nmx_device_pool_trim: a co-tenant of the GPU cannot reclaim it); returns how many staging
    pools were freed."""
    n = 0
    libs = {}
    for key in [k for k, p in _STAGING.items() if p.users <= 0]:
        pool = _STAGING.pop(key)
        libs[id(pool.lib)] = pool.lib
        pool.close()
        n += 1
    for p in _STAGING.values():
        libs[id(p.lib)] = p.lib
    for lib in libs.values():
        trim_device_pool(lib)
    return n


def trim_device_pool(lib=None, keep_bytes: int = 0) -> int:
    """Idle device blocks of destroyed plans back to the driver until at most ``keep_bytes`` stay cached -> bytes freed."""
    lib = lib if lib is not None else _lib.get_library()
    freed = C.c_int64(0)
    lib.check(lib.lib.nmx_device_pool_trim(int(keep_bytes), C.byref(freed)))
    return int(freed.value)


def _free_all_staging() -> None:   # atexit
    for key in list(_STAGING):
        try:
            pool = _STAGING.pop(key)
            pool.close()
            pool.lib.lib.nmx_device_pool_trim(0, None)
        except Exception:
            pass


atexit.register(_free_all_staging)


_scratch_tls = threading.local()


def _offset_scratch(rows: int, cols: int) -> np.ndarray:
    """A C-ordered float64 [rows, cols] scratch array of the calling thread (`HotPathEngine._host_offsets`)."""
    buf = getattr(_scratch_tls, "buf", None)
    if buf is None or buf.size < rows * cols:
        buf = _scratch_tls.buf = np.empty(max(rows * cols, 1 << 16), np.float64)
    return buf[:rows * cols].reshape(rows, cols)


class _Pinned:
    """Page-locked staging arrays (nmx_host_alloc), grown on demand and reused across calls."""

    def __init__(self, lib, key=None) -> None:
        self.lib, self._bufs, self.users, self.key = lib, {}, 0, key

    def array(self, name: str, shape, dtype) -> np.ndarray:
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr, cap = self._bufs.get(name, (None, 0))
        if cap < n:
            if ptr:
                self.lib.lib.nmx_host_free(ptr)
            p = C.c_void_p()
            self.lib.check(self.lib.lib.nmx_host_alloc(n + n // 8 + 64, C.byref(p)))
            ptr, cap = p.value, n + n // 8 + 64
            self._bufs[name] = (ptr, cap)
        buf = (C.c_char * n).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self) -> None:
        for ptr, _ in self._bufs.values():
            if ptr:
                self.lib.lib.nmx_host_free(ptr)
        self._bufs = {}


def staging_thread(edges, stage, ctrs, T: int, failed: list) -> threading.Thread:
    """The staging thread of a pipelined batch (nmx_plan_set_pipeline), not started: ``stage(a, b)`` for the consecutive
    sample ranges of ``edges()``, publishing after each in ``c[0]`` of every counter array of ``ctrs`` how many samples
    are in place.  On failure the exception goes into ``failed`` -- reported by the caller's thread -- and T is
    published: the plans run out on what is there."""
    def work():
        try:
            e = edges()
            for a, b in zip(e[:-1], e[1:]):
                stage(a, b)
                for c in ctrs:
                    c[0] = b
        except BaseException as exc:   # noqa: BLE001
            failed.append(exc)
            for c in ctrs:
                c[0] = T

    return threading.Thread(target=work, daemon=True)
