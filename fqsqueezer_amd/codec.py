"""ctypes binding of the C ABI in include/fqsx.h (libfqsx.so, HIP/gfx950).

The product path has no CPU implementation: constructing a DnaCodec without the
built HIP library or without a GPU raises.  (tests/emu passes the path of the
host-emulation build of the *same kernels* explicitly; nothing in this package
ever selects it.)
"""
from __future__ import annotations

import ctypes as C
import os
import zlib
from typing import List, Optional

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_PKG, "libfqsx.so")

STAT_NAMES = ["gprobe", "gslot", "lprobe", "lslot", "gins", "gins_slot", "siv_words", "ctx_slots",
              "coded", "lins", "mail", "bases", "siv_saved", "dec_refetch", "ins_windows", "ins_windows_in_order"]


class FqsxError(RuntimeError):
    pass


class LengthMismatch(ValueError):
    """a record whose quality line differs in length from its base line, where that cannot be held"""


_P, _INT, _U32, _U64, _HDR = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_char_p
_OUT, _U64S, _MS, _IN = C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_char_p)
_ID_ENCODE = [_P, _P, _P, _U32, _INT, _OUT, _U64S]
_ID_DECODE = [_P, _IN, _P, _U32, _INT, _OUT, _OUT]

# Every function of include/fqsx.h this module calls: name -> (restype, argtypes).  _OUT: a handle or a pointer the library
# hands back; _IN with the _P behind it: T input streams and their lengths (_pack); _OUT, _U64S at the end of an encoder's
# list: its T output streams (_Handle._collect).  (sharded.py binds the fqsx_shard_* / fqsx_rccl_* calls it makes itself.)
_ABI = {
    "fqsx_dna_create": (_INT, [_HDR, _INT, _OUT]),
    "fqsx_dna_create_on_partition": (_INT, [_HDR, _INT, _U32, _U32, _OUT]),
    "fqsx_dna_destroy": (None, [_P]),
    "fqsx_dna_use_chunked_tables": (_INT, [_P]),
    "fqsx_dna_encode_block": (_INT, [_P, _P, _P, _U32, _U32, _OUT, _U64S]),
    "fqsx_dna_encode_block_dev": (_INT, [_P, _P, _P, _P, _U32, _U32, _OUT, _U64S]),
    "fqsx_dna_decode_block": (_INT, [_P, _IN, _P, _P, _U32, _U32, _P]),
    "fqsx_dna_decode_block_dev": (_INT, [_P, _IN, _P, _P, _U32, _U32, _OUT]),
    "fqsx_dna_stats": (_INT, [_P, _U64S]),
    "fqsx_dna_capacity": (_INT, [_P, _U64S]),
    "fqsx_dna_set_profiling": (_INT, [_P, _INT]),
    "fqsx_dna_kernel_times": (_INT, [_P, _MS]),
    "fqsx_qual_create": (_INT, [_HDR, _INT, _OUT]),
    "fqsx_qual_destroy": (None, [_P]),
    "fqsx_qual_encode_block": (_INT, [_P, _P, _P, _U32, _OUT, _U64S]),
    "fqsx_qual_encode_block_dev": (_INT, [_P, _P, _P, _P, _U32, _OUT, _U64S]),
    "fqsx_qual_decode_block": (_INT, [_P, _IN, _P, _P, _U32, _P]),
    "fqsx_qual_decode_block_dev": (_INT, [_P, _IN, _P, _P, _U32, _OUT]),
    "fqsx_qual_contexts": (_INT, [_P, _P]),
    "fqsx_qual_set_profiling": (_INT, [_P, _INT]),
    "fqsx_qual_kernel_times": (_INT, [_P, _MS]),
    "fqsx_meta_create": (_INT, [_U32, _OUT]),
    "fqsx_meta_destroy": (None, [_P]),
    "fqsx_meta_encode_block_pe": (_INT, [_P, _P, _U32, _INT, _OUT, _U64S]),
    "fqsx_meta_decode_block": (_INT, [_P, _IN, _P, _U32, _INT, _P]),
    "fqsx_id_create": (_INT, [_HDR, _OUT]),
    "fqsx_id_destroy": (None, [_P]),
    "fqsx_id_encode_block": (_INT, _ID_ENCODE),
    "fqsx_id_decode_block": (_INT, _ID_DECODE),
    "fqsx_idg_create": (_INT, [_HDR, _INT, _OUT]),
    "fqsx_idg_destroy": (None, [_P]),
    "fqsx_idg_encode_block": (_INT, _ID_ENCODE),
    "fqsx_idg_encode_block_dev": (_INT, [_P, _P, _P, _P, _U32, _INT, _OUT, _U64S]),
    "fqsx_idg_decode_block": (_INT, _ID_DECODE),
    "fqsx_idg_decode_block_dev": (_INT, [_P, _IN, _P, _U32, _INT, _OUT, _OUT, _U64S]),
    "fqsx_idg_error_kind": (_INT, [_P]),
    "fqsx_idg_stats": (_INT, [_P, _U64S]),
    "fqsx_idg_state": (_INT, [_P, _P]),
    "fqsx_idg_set_profiling": (_INT, [_P, _INT]),
    "fqsx_idg_kernel_times": (_INT, [_P, _MS]),
    "fqsx_idg_separator_times": (_INT, [_P, _MS]),
    "fqsx_sort_order": (_INT, [_P, _P, _U32, _INT, _P, _P]),
    "fqsx_sort_order_batched": (_INT, [_P, _P, _U32, _INT, _U64, _P, _P, C.POINTER(_U32)]),
    "fqsx_fastq_create": (_INT, [_INT, _U64, _OUT]),
    "fqsx_fastq_destroy": (None, [_P]),
    "fqsx_fastq_max_chunk": (_U64, [_P]),
    "fqsx_fastq_index": (_INT, [_P, _P, _U64, _U64S]),
    "fqsx_fastq_columns": (_INT, [_P] * 8),
    "fqsx_fastq_columns_into": (_INT, [_P] * 6),
    "fqsx_fastq_set_profiling": (_INT, [_P, _INT]),
    "fqsx_fastq_kernel_times": (_INT, [_P, _MS]),
    "fqsx_bgzf_scan": (_INT, [_P, _U64, _U32, _P, _P, _U64S]),
    "fqsx_bgzf_inflate": (_INT, [_P, _P, _U64, _P, _U32, _P, _U64S]),
    "fqsx_fastq_index_bgzf": (_INT, [_P, _P, _U64, _P, _U32, _U64, _U64S, _U64S]),
    "fqsx_fastq_inflate_times": (_INT, [_P, _MS]),
    "fqsx_cols_create": (_INT, [_INT, _OUT]),
    "fqsx_cols_destroy": (None, [_P]),
    "fqsx_cols_info": (_INT, [_P, _U64S]),
    "fqsx_cols_gather": (_INT, [_P, _P, _P, _U32, _P, _OUT, _OUT, _OUT]),
    "fqsx_cols_bases": (_INT, [_P, _P]),
    "fqsx_cols_sort_order": (_INT, [_P, _P, _P, _U64S]),
    "fqsx_cols_download": (_INT, [_P, _P, _P, _U64]),
    "fqsx_cols_set_profiling": (_INT, [_P, _INT]),
    "fqsx_cols_kernel_times": (_INT, [_P, _MS]),
    "fqsx_cols_keep_ids": (_INT, [_P]),
    "fqsx_cols_gather_ids": (_INT, [_P, _P, _P, _U32, _P, _OUT, _OUT]),
    "fqsx_cols_id_info": (_INT, [_P, _U64S]),
    "fqsx_cols_id_survey": (_INT, [_P, _U64S]),
    "fqsx_cols_id_kernel_times": (_INT, [_P, _MS]),
    "fqsx_fqtext_create": (_INT, [_INT, _OUT]),
    "fqsx_fqtext_destroy": (None, [_P]),
    "fqsx_fqtext_block": (_INT, [_P, _U32, _INT, _P, _P, _INT, _U64, _P, _P, _INT, _P, _U64S]),
    "fqsx_fqtext_download": (_INT, [_P, _INT, _P]),
    "fqsx_fqtext_set_profiling": (_INT, [_P, _INT]),
    "fqsx_fqtext_kernel_times": (_INT, [_P, _MS]),
    "fqsx_last_error": (C.c_char_p, []),
    "fqsx_version": (C.c_char_p, []),
}


def _load(path: str):
    if not os.path.exists(path):
        raise FqsxError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    try:  # PyTorch ships its own ROCm runtime: load it first so the process has ONE HIP runtime
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (restype, argtypes) in _ABI.items():
        f = getattr(lib, name, None)   # (tools/ab_bench.py also loads builds that predate the newer entry points)
        if f is not None:
            f.restype, f.argtypes = restype, argtypes
    return lib


_libs = {}


def load_library(path: Optional[str] = None):
    path = path or DEFAULT_LIB
    if path not in _libs:
        _libs[path] = _load(path)
    return _libs[path]


def _error(lib, name: str, rc: int, text: Optional[str] = None, fmt: str = "{name}: {rc}: {text}") -> FqsxError:
    """text: the library's (fqsx_last_error) unless the caller has its own; `.code` is the return code"""
    e = FqsxError(fmt.format(name=name, rc=rc, text=lib.fqsx_last_error().decode() if text is None else text))
    e.code = rc
    return e


def _pack(streams, T: int):
    """T input streams as the decode entry points take them: (array of T pointers, their uint64 lengths)"""
    return (C.c_char_p * T)(*[bytes(x) for x in streams]), np.array([len(x) for x in streams], dtype=np.uint64)


class _Handle:
    """An object of the library behind its opaque pointer: made by one fqsx_*_create, released once by its fqsx_*_destroy."""
    _lib = _h = None

    def _open(self, lib_path: Optional[str], create: str, destroy: str, *args, **error) -> None:
        self._lib = load_library(lib_path)
        self._h, self._destroy = C.c_void_p(), destroy
        self._call(create, *args, C.byref(self._h), **error)

    def _call(self, name: str, *args, text=None, fmt: str = "{name}: {rc}: {text}") -> None:
        """text: None (the library's), the caller's own, or a function of the return code that gives it"""
        rc = getattr(self._lib, name)(*args)
        if rc:
            raise self._error(name, rc, text(rc) if callable(text) else text, fmt)

    def _error(self, name: str, rc: int, text: Optional[str], fmt: str) -> FqsxError:
        return _error(self._lib, name, rc, text, fmt)

    def _outputs(self, T: int) -> None:
        """the T output streams of an encoder's block, owned by the library until the next call"""
        self.T = T
        self._streams = (C.c_void_p * T)()
        self._lens = (C.c_uint64 * T)()

    def _collect(self) -> List[bytes]:
        return [C.string_at(self._streams[w], self._lens[w]) if self._lens[w] else b"" for w in range(self.T)]

    def _stream_bytes(self) -> int:
        return sum(self._lens[w] for w in range(self.T))

    def close(self) -> None:
        if self._h:
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DnaCodec(_Handle):
    """One .fqs file's DNA-stream encoder state on one GPU (fqsx_dna_*)."""

    def __init__(self, header: bytes, device: int = 0, lib_path: Optional[str] = None, partition: Optional[tuple] = None,
                 chunked_tables: bool = False):
        """partition = (k, n): confine the codec's kernels to the k-th of n equal sets of compute units (several files at once on one GPU).
        chunked_tables: the capacity mode (fqsx_dna_use_chunked_tables): a growth never holds the old and the new table side by side."""
        if len(header) != 17:
            raise ValueError("header must be the 17 .fqs parameter bytes")
        if partition is None:
            self._open(lib_path, "fqsx_dna_create", "fqsx_dna_destroy", bytes(header), device)
        else:
            self._open(lib_path, "fqsx_dna_create_on_partition", "fqsx_dna_destroy", bytes(header), device, partition[0], partition[1])
        if chunked_tables:
            self._call("fqsx_dna_use_chunked_tables", self._h, fmt="{name}: {text}")
        self._outputs(header[4])

    def encode_block(self, bases: np.ndarray, read_off: np.ndarray, generation: int) -> List[bytes]:
        """Host-buffer entry point: returns the T per-worker DNA streams of the block."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        self._call("fqsx_dna_encode_block", self._h, bases.ctypes.data, read_off.ctypes.data, len(read_off) - 1,
                   generation, self._streams, self._lens)
        return self._collect()

    def encode_block_dev(self, d_bases_ptr: int, d_off_ptr: int, read_off: np.ndarray, generation: int,
                         collect: bool = True):
        """Device-resident entry point (inputs already in HBM)."""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        self._call("fqsx_dna_encode_block_dev", self._h, d_bases_ptr, d_off_ptr, read_off.ctypes.data,
                   len(read_off) - 1, generation, self._streams, self._lens)
        return self._collect() if collect else self._stream_bytes()

    def decode_block(self, streams, read_off: np.ndarray, generation: int) -> np.ndarray:
        """Inverse of encode_block: the T DNA streams of a block + read offsets -> concatenated base bytes."""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        arr, lens = _pack(streams, self.T)
        out = np.zeros(max(1, int(read_off[-1])), dtype=np.uint8)
        self._call("fqsx_dna_decode_block", self._h, arr, lens.ctypes.data, read_off.ctypes.data, len(read_off) - 1,
                   generation, out.ctypes.data)
        return out[:int(read_off[-1])]

    def decode_block_dev(self, streams, read_off: np.ndarray, generation: int) -> int:
        """The same, leaving the block in device memory: returns the device pointer (the codec's output buffer, valid until
        the next call on this codec)."""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        arr, lens = _pack(streams, self.T)
        d_out = C.c_void_p()
        self._call("fqsx_dna_decode_block_dev", self._h, arr, lens.ctypes.data, read_off.ctypes.data, len(read_off) - 1,
                   generation, C.byref(d_out))
        return d_out.value or 0

    def stats(self) -> dict:
        a = (C.c_uint64 * 64)()
        self._call("fqsx_dna_stats", self._h, a)
        d = dict(zip(STAT_NAMES, list(a)))
        d["timers"] = list(a)[16:64]
        return d

    def capacity(self) -> dict:
        """Table occupancy and device memory (fqsx_dna_capacity)."""
        a = (C.c_uint64 * 16)()
        self._call("fqsx_dna_capacity", self._h, a)
        d = {"smers": a[0], "bmers": a[1], "smer_slots": a[2], "bmer_slots": a[3], "siv_bytes": a[4], "ctx_slots": a[5],
             "contexts": a[6], "device_bytes": a[7], "device_bytes_peak": a[8], "growths": a[9], "pairs": a[10], "pair_slots": a[11],
             "table_bytes_held": a[13], "pair_bytes_held": a[14], "siv_bytes_held": a[15]}
        d["bytes_per_bmer"] = round(a[3] * a[12] / a[1], 2) if a[1] else 0.0
        d["bytes_per_smer"] = round(a[2] * a[12] / a[0], 2) if a[0] else 0.0
        return d

    def set_profiling(self, on: bool) -> None:
        self._lib.fqsx_dna_set_profiling(self._h, int(on))

    def kernel_times(self) -> dict:
        a = (C.c_double * 6)()
        self._lib.fqsx_dna_kernel_times(self._h, a)
        return {"encode_ms": a[0], "insert_ms": a[1], "other_ms": a[2],
                "encode_launches": int(a[3]), "insert_launches": int(a[4]), "other_launches": int(a[5])}


class MetaCodec(_Handle):
    """Host-side read-length stream of the container (fqsx_meta_*).  (The host coders never set the library's error text.)"""

    def __init__(self, threads: int, lib_path: Optional[str] = None):
        self._open(lib_path, "fqsx_meta_create", "fqsx_meta_destroy", threads, fmt="{name} failed")
        self._outputs(threads)

    def encode_block(self, read_len: np.ndarray, paired: bool = False) -> List[bytes]:
        read_len = np.ascontiguousarray(read_len, dtype=np.uint32)
        self._call("fqsx_meta_encode_block_pe", self._h, read_len.ctypes.data, len(read_len), int(paired), self._streams, self._lens,
                   fmt="fqsx_meta_encode_block failed")
        return self._collect()

    def decode_block(self, streams, n_reads: int, paired: bool = False) -> np.ndarray:
        """Inverse of encode_block: the T meta streams of a block -> its n_reads read lengths (an instance encodes or decodes a
        file, never both)."""
        arr, lens = _pack(streams, self.T)
        out = np.zeros(max(1, n_reads), dtype=np.uint32)
        self._call("fqsx_meta_decode_block", self._h, arr, lens.ctypes.data, n_reads, int(paired), out.ctypes.data,
                   text="malformed or truncated meta stream")
        return out[:n_reads]


def sort_order(bases: np.ndarray, read_off: np.ndarray, device: int = 0, lib_path: Optional[str] = None,
               max_batch_bases: int = 0, stats: Optional[dict] = None) -> List[np.ndarray]:
    """Read order of `fqs e -om s` (fqsx_sort_order: GPU radix sort + ranks, host replay of std::sort per bin).
    Returns one index array per non-empty bin, in bin order -- the same shape hostpipe.sorted_order_exact returns.
    max_batch_bases > 0: bounded device memory (fqsx_sort_order_batched: bins packed into batches of at most that many bases)."""
    lib = load_library(lib_path)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
    n = len(read_off) - 1
    order = np.empty(max(n, 1), dtype=np.uint32)
    bins = np.zeros(257, dtype=np.uint32)
    nb = C.c_uint32(0)
    rc = lib.fqsx_sort_order_batched(bases.ctypes.data, read_off.ctypes.data, n, device, max_batch_bases, order.ctypes.data, bins.ctypes.data, C.byref(nb))
    if rc:
        raise _error(lib, "fqsx_sort_order", rc)
    if stats is not None:
        stats["batches"] = nb.value
    return _bins_of(order, bins)


def _bins_of(order: np.ndarray, bins: np.ndarray) -> List[np.ndarray]:
    """order_out / bin_start of the fqsx_*sort_order calls as one index array per non-empty bin"""
    return [order[bins[b]:bins[b + 1]].astype(np.int64) for b in range(256) if bins[b + 1] > bins[b]]


class IdCodec(_Handle):
    """Read-id stream of the container (header byte 7 = id mode).  device = None: the host coder (fqsx_id_*, one host thread per
    worker); device = ordinal: the GPU coder (fqsx_idg_*, one wavefront per worker) -- the same bytes.  Both flavours decode too."""

    def __init__(self, header: bytes, lib_path: Optional[str] = None, device: Optional[int] = None):
        self._mode = header[7]   # 0 lossless, 1 instrument
        self._gpu = device is not None
        if self._gpu:
            self._open(lib_path, "fqsx_idg_create", "fqsx_idg_destroy", bytes(header), device)
        else:
            self._open(lib_path, "fqsx_id_create", "fqsx_id_destroy", bytes(header), fmt="{name} failed")
        self._outputs(header[4])

    def _error(self, name: str, rc: int, text: Optional[str], fmt: str) -> FqsxError:
        """A block's error has `staging`.  GPU flavour: True if the kernel met an id beyond its staging sizes or its list of
        instrument names (fqsx_idg_error_kind 5 and 6); its models have moved by then, so the file goes on with the host
        flavour (IdFallback)."""
        e = super()._error(name, rc, text, fmt)
        if "_block" in name:
            e.staging = self._gpu and rc == -5 and self._lib.fqsx_idg_error_kind(self._h) in (5, 6)
        return e

    @property
    def on_device(self) -> bool:
        """the GPU flavour"""
        return self._gpu

    def encode_block(self, ids: np.ndarray, id_off: np.ndarray, paired: bool = False) -> List[bytes]:
        ids = np.ascontiguousarray(ids, dtype=np.uint8)
        id_off = np.ascontiguousarray(id_off, dtype=np.uint64)
        self._call("fqsx_idg_encode_block" if self._gpu else "fqsx_id_encode_block", self._h, ids.ctypes.data, id_off.ctypes.data,
                   len(id_off) - 1, int(paired), self._streams, self._lens,
                   text=None if self._gpu else lambda rc: self._host_refusal(ids, id_off, paired))
        return self._collect()

    def encode_block_dev(self, d_ids: int, d_off: int, id_off: np.ndarray, paired: bool = False) -> List[bytes]:
        """GPU flavour only: encode_block for a block in device memory (DeviceColumns.ids_dev: the device pointers of its id lines
        and of their offsets, and the offsets on the host).  The same streams, errors and `staging` as encode_block's."""
        if not self._gpu:
            raise FqsxError("encode_block_dev: the host id coder reads host arrays")
        id_off = np.ascontiguousarray(id_off, dtype=np.uint64)
        self._call("fqsx_idg_encode_block_dev", self._h, d_ids or None, d_off or None, id_off.ctypes.data, len(id_off) - 1, int(paired),
                   self._streams, self._lens)
        return self._collect()

    def _host_refusal(self, ids: np.ndarray, id_off: np.ndarray, paired: bool) -> str:
        """The host flavour never sets the library's error text: its one return code gets its message here."""
        if paired and (len(id_off) - 1) & 1:
            return "a paired block with an odd number of reads"
        # (the two reasons for which the host coder refuses an id, fqsx_host.cpp id_lossless / id_instrument)
        ends = np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum((ids == 0x2E) | (ids == 0x20) | (ids == 0x3A), out=ends[1:])
        off = id_off.astype(np.int64)
        if self._mode == 1 and bool((ends[off[1:]] == ends[off[:-1]]).any()):
            return "no instrument name: an id line without '.', ' ' or ':'"
        if len(ids) and int(ids.max()) >= 128:
            return "byte outside the 128-symbol alphabet in an id line"
        return "bad argument"

    @staticmethod
    def _host_stream_error(rc: int) -> str:
        return "a worker's stream is shorter than 8 bytes or a bad argument" if rc == -1 else "malformed or truncated id stream"

    def _decode(self, name: str, streams, n_reads: int, paired: bool, *out) -> None:
        arr, lens = _pack(streams, self.T)
        self._call(name, self._h, arr, lens.ctypes.data, n_reads, int(paired), *[C.byref(x) for x in out],
                   text=None if self._gpu else self._host_stream_error)

    def decode_block(self, streams, n_reads: int, paired: bool = False):
        """Inverse of encode_block: the T id streams of a block -> (ids uint8[], id_off uint64[n_reads + 1]), the id lines the
        reference's decoder writes, each with its line feed, in block order (an instance encodes or decodes a file, never both).
        GPU flavour: FqsxError whose `staging` is True if a line is beyond what the kernel stages (the host flavour has no limits)."""
        ids, off = C.c_void_p(), C.c_void_p()
        self._decode("fqsx_idg_decode_block" if self._gpu else "fqsx_id_decode_block", streams, n_reads, paired, ids, off)
        id_off = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(n_reads + 1,)).copy()
        n = int(id_off[-1])
        out = np.ctypeslib.as_array(C.cast(ids, C.POINTER(C.c_uint8)), shape=(max(n, 1),))[:n].copy()
        return out, id_off

    def decode_block_dev(self, streams, n_reads: int, paired: bool = False):
        """GPU flavour only: decode_block leaving the block in device memory.  Returns (d_ids, d_id_len, id_bytes): the device
        pointers of the id lines back to back and of their n_reads uint32 lengths (both the codec's, valid until its next call)
        and the bytes of the lines.  Errors as decode_block's, `staging` included."""
        if not self._gpu:
            raise FqsxError("decode_block_dev: the host id decoder has no device output")
        ids, idl, nb = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._decode("fqsx_idg_decode_block_dev", streams, n_reads, paired, ids, idl, nb)
        return ids.value or 0, idl.value or 0, int(nb.value)

    def error_kind(self) -> int:
        """GPU flavour: what the kernel reported in the last block (fqsx_idg_error_kind; 0 = nothing)"""
        return int(self._lib.fqsx_idg_error_kind(self._h)) if self._gpu else 0

    def _kernel_coder(self, name: str, *args) -> None:
        if not self._gpu:
            raise FqsxError(f"{name} failed")
        self._call(name, self._h, *args, fmt="{name} failed")

    def stats(self) -> dict:
        """GPU flavour: how often the decoder had to grow (fqsx_idg_stats) and its capacities."""
        a = (C.c_uint64 * 8)()
        self._kernel_coder("fqsx_idg_stats", a)
        return dict(zip(["retries", "grow_small", "grow_big", "grow_out", "small_slots", "big_slots", "out_bytes"], [int(x) for x in a]))

    def state(self) -> np.ndarray:
        """GPU flavour: (T, 3) models in the small table, in the big table and move-to-front names per worker after the last block."""
        a = np.zeros(4 * self.T, dtype=np.uint32)
        self._kernel_coder("fqsx_idg_state", a.ctypes.data)
        return a.reshape(self.T, 4)[:, :3].copy()

    def set_profiling(self, on: bool) -> None:
        self._lib.fqsx_idg_set_profiling(self._h, int(on))

    def kernel_times(self) -> dict:
        a = (C.c_double * 2)()
        self._lib.fqsx_idg_kernel_times(self._h, a)
        b = (C.c_double * 2)()
        self._lib.fqsx_idg_separator_times(self._h, b)
        return {"ms": a[0], "launches": int(a[1]), "separators_ms": b[0], "separators_launches": int(b[1])}


class IdFallback:
    """The id coder of one file: the GPU kernel, or -- once the kernel reports `staging` (IdCodec._error) -- the host coder,
    brought to the same state by coding again, in order, the blocks the kernel has coded.  The blocks already done stay as they
    are: both coders write and read the same bytes.  The user says what coding a block means: code(codec, what, held), where
    `what` is all that is kept of a block to code it again and `held`, given on its first run only, what the caller has at hand
    then.  fqsfile keeps a block's index array and cuts its id columns again; fqsread keeps its streams."""

    def __init__(self, header: bytes, device: int, lib_path: Optional[str], gpu_ids: bool, code):
        self._header, self._lib_path, self._code = header, lib_path, code
        self.codec = IdCodec(header, lib_path=lib_path, device=device if gpu_ids else None)   # the live one (stats())
        self.on_gpu, self.fell_back = gpu_ids, False
        self._seen = []   # `what` of the blocks coded on the GPU so far

    def run(self, what, held=None):
        if self.on_gpu:
            try:
                out = self._code(self.codec, what, held)
                self._seen.append(what)
                return out
            except FqsxError as e:
                if not getattr(e, "staging", False):
                    raise
            self.codec.close()
            self.codec = IdCodec(self._header, lib_path=self._lib_path)
            self.on_gpu, self.fell_back = False, True
            for w in self._seen:
                self._code(self.codec, w, None)
            self._seen = []
        return self._code(self.codec, what, held)

    def close(self) -> None:
        self.codec.close()


class QualCodec(_Handle):
    """Quality-stream coder on the GPU (fqsx_qual_*): one instance encodes or decodes a file, never both."""

    def __init__(self, header: bytes, device: int = 0, lib_path: Optional[str] = None):
        self._open(lib_path, "fqsx_qual_create", "fqsx_qual_destroy", bytes(header), device)
        self._outputs(header[4])

    def encode_block(self, quals: np.ndarray, read_off: np.ndarray) -> List[bytes]:
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        self._call("fqsx_qual_encode_block", self._h, quals.ctypes.data, read_off.ctypes.data, len(read_off) - 1,
                   self._streams, self._lens)
        return self._collect()

    def encode_block_dev(self, d_quals_ptr: int, d_off_ptr: int, read_off: np.ndarray, collect: bool = False):
        """Device-resident entry point; returns the total stream bytes of the block or -- collect -- its T streams."""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        self._call("fqsx_qual_encode_block_dev", self._h, d_quals_ptr, d_off_ptr, read_off.ctypes.data, len(read_off) - 1,
                   self._streams, self._lens)
        return self._collect() if collect else self._stream_bytes()

    def decode_block(self, streams, read_off: np.ndarray) -> np.ndarray:
        """Inverse of encode_block: the T quality streams of a block + read offsets -> concatenated quality bytes (ASCII)."""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        arr, lens = _pack(streams, self.T)
        out = np.zeros(max(1, int(read_off[-1])), dtype=np.uint8)
        self._call("fqsx_qual_decode_block", self._h, arr, lens.ctypes.data, read_off.ctypes.data, len(read_off) - 1, out.ctypes.data)
        return out[:int(read_off[-1])]

    def decode_block_dev(self, streams, read_off: np.ndarray) -> int:
        """The same, leaving the block in device memory: returns the device pointer (valid until the next call)."""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        arr, lens = _pack(streams, self.T)
        d_out = C.c_void_p()
        self._call("fqsx_qual_decode_block_dev", self._h, arr, lens.ctypes.data, read_off.ctypes.data, len(read_off) - 1, C.byref(d_out))
        return d_out.value or 0

    def contexts(self) -> dict:
        """Contexts stored per worker and the slots per worker of the context table (fqsx_qual_contexts)."""
        a = np.zeros(self.T + 1, dtype=np.uint64)
        self._call("fqsx_qual_contexts", self._h, a.ctypes.data)
        return {"per_worker": [int(x) for x in a[:self.T]], "slots_per_worker": int(a[self.T])}

    def set_profiling(self, on: bool) -> None:
        self._lib.fqsx_qual_set_profiling(self._h, int(on))

    def kernel_times(self) -> dict:
        a = (C.c_double * 2)()
        self._lib.fqsx_qual_kernel_times(self._h, a)
        return {"encode_ms": a[0], "encode_launches": int(a[1])}   # (of a decoding instance: its decode launches)


FASTQ_PASSES = ["count", "scan_tiles", "index", "lengths", "scan_rtiles", "offsets", "gather"]


class FastqParser(_Handle):
    """FASTQ text to columns on the GPU (fqsx_fastq_*): one chunk of text per call."""

    def __init__(self, device: int = 0, lib_path: Optional[str] = None, max_chunk_bytes: int = 0):
        self._open(lib_path, "fqsx_fastq_create", "fqsx_fastq_destroy", device, max_chunk_bytes)
        self.max_chunk_bytes = int(self._lib.fqsx_fastq_max_chunk(self._h))

    def index(self, text: np.ndarray) -> dict:
        """Upload a chunk (uint8 array) and find its records: sizes for columns()."""
        a = (C.c_uint64 * 8)()
        self._call("fqsx_fastq_index", self._h, text.ctypes.data if len(text) else None, len(text), a)
        return {"records": int(a[0]), "consumed": int(a[1]), "id_bytes": int(a[2]), "bases": int(a[3]), "quals": int(a[4]),
                "max_id_line": int(a[5]), "length_mismatch": bool(a[6]), "line_feeds": int(a[7])}

    def index_bgzf(self, members: np.ndarray, member_off: np.ndarray, carry: int = 0) -> dict:
        """index() of the chunk that is the last `carry` bytes of the previous chunk's text, kept on the device, followed by the
        text of the BGZF members `members` (uint8; member i begins at member_off[i], uint64), inflated on the GPU.  The dict also
        has "text_bytes", the chunk's size.  A damaged member: FqsxError with `.member` (its index) and `.kind` (INFLATE_KINDS)."""
        a, info = (C.c_uint64 * 8)(), (C.c_uint64 * 4)()
        member_off = np.ascontiguousarray(member_off, dtype=np.uint64)
        try:
            self._call("fqsx_fastq_index_bgzf", self._h, members.ctypes.data if len(members) else None, len(members),
                       member_off.ctypes.data if len(member_off) else None, len(member_off), carry, a, info)
        except FqsxError as e:
            if info[1]:
                e.member, e.kind = int(info[0]), INFLATE_KINDS[int(info[1])]
            raise
        return {"records": int(a[0]), "consumed": int(a[1]), "id_bytes": int(a[2]), "bases": int(a[3]), "quals": int(a[4]),
                "max_id_line": int(a[5]), "length_mismatch": bool(a[6]), "line_feeds": int(a[7]), "text_bytes": carry + int(info[2])}

    def inflate_times(self) -> dict:
        a = (C.c_double * 2)()
        self._lib.fqsx_fastq_inflate_times(self._h, a)
        return {"ms": a[0], "launches": int(a[1])}

    def columns(self, info: dict):
        """(ids, id_off, bases, read_off, quals, qual_off, plus_len) of the chunk indexed last."""
        n = info["records"]
        ids, bases, quals = (np.empty(info[k], dtype=np.uint8) for k in ("id_bytes", "bases", "quals"))
        id_off, read_off, qual_off = (np.zeros(n + 1, dtype=np.uint64) for _ in range(3))
        plus_len = np.empty(n, dtype=np.uint32)
        self._call("fqsx_fastq_columns", self._h, ids.ctypes.data, id_off.ctypes.data, bases.ctypes.data, read_off.ctypes.data,
                   quals.ctypes.data, qual_off.ctypes.data, plus_len.ctypes.data)
        return ids, id_off, bases, read_off, quals, qual_off, plus_len

    def columns_into(self, info: dict, store: "DeviceColumns"):
        """(ids, id_off, read_off, plus_len) of the chunk indexed last; its base and quality columns are appended to `store`
        without leaving the device -- its id lines too if the store keeps ids (`ids` is then empty).  FqsxError, the store unchanged:
        a record whose quality line differs in length from its base line."""
        n = info["records"]
        ids = np.empty(0 if store.keeps_ids else info["id_bytes"], dtype=np.uint8)   # (a store that keeps ids: no id byte comes to the host)
        id_off, read_off = (np.zeros(n + 1, dtype=np.uint64) for _ in range(2))
        plus_len = np.empty(n, dtype=np.uint32)
        self._call("fqsx_fastq_columns_into", self._h, store._h, None if store.keeps_ids else ids.ctypes.data, id_off.ctypes.data,
                   read_off.ctypes.data, plus_len.ctypes.data)
        return ids, id_off, read_off, plus_len

    def set_profiling(self, on: bool) -> None:
        self._lib.fqsx_fastq_set_profiling(self._h, int(on))

    def kernel_times(self) -> dict:
        a = (C.c_double * 14)()
        self._lib.fqsx_fastq_kernel_times(self._h, a)
        return {name: {"ms": a[k], "launches": int(a[7 + k])} for k, name in enumerate(FASTQ_PASSES)}


# the kinds of damage the inflate kernel tells apart (csrc/fqsx_inflate.h: INF_E_*), by their number
INFLATE_KINDS = ["none", "reserved block type", "stored LEN/NLEN mismatch", "over-subscribed or incomplete code", "invalid symbol",
                 "distance before the member's start", "output beyond ISIZE", "input exhausted", "ISIZE mismatch", "CRC mismatch",
                 "no BGZF member header"]

FQTEXT_PASSES = ["sizes", "scan_tiles", "offsets", "scatter"]


class FastqText(_Handle):
    """Columns to FASTQ text on the GPU (fqsx_fqtext_*): one container block per call, the text `fqs d` writes for it."""

    def __init__(self, device: int = 0, lib_path: Optional[str] = None):
        self._open(lib_path, "fqsx_fqtext_create", "fqsx_fqtext_destroy", device)
        self.text_bytes = (0, 0)

    def block(self, read_off: np.ndarray, d_bases: int, d_quals: Optional[int] = None, ids=None, id_len=None, id_bytes: Optional[int] = None,
              paired: bool = False, qual_fill: int = 0):
        """Assemble the block whose reads lie under read_off (uint64[n + 1], from 0) in the device columns d_bases / d_quals
        (device pointers; d_quals None: every quality is the byte qual_fill).  ids / id_len: device pointers with id_bytes (what
        IdCodec.decode_block_dev returns), or host arrays (uint8 id lines back to back, their uint32 lengths), or None: every id
        line is "@\n".  Returns (n0, n1), the bytes of the two outputs (n1 = 0 unless paired).  FqsxError with `.code` -1 for
        inputs that contradict each other, -5 for a range outside a buffer; the previous block's text stays as it was."""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n = len(read_off) - 1
        on_device, keep = 0, None
        if ids is None:
            p_ids, p_len, nb = None, None, 0
        elif isinstance(ids, np.ndarray):
            keep = (np.ascontiguousarray(ids, dtype=np.uint8), np.ascontiguousarray(id_len, dtype=np.uint32))
            if len(keep[1]) != n:
                raise ValueError("id_len must have one entry per read")
            p_ids, p_len = keep[0].ctypes.data, keep[1].ctypes.data
            nb = len(keep[0]) if id_bytes is None else int(id_bytes)
        else:
            p_ids, p_len, nb, on_device = int(ids), int(id_len), int(id_bytes), 1
        out = (C.c_uint64 * 2)()
        self._call("fqsx_fqtext_block", self._h, n, int(paired), p_ids, p_len, on_device, nb, d_bases or None, d_quals or None,
                   int(qual_fill), read_off.ctypes.data, out)
        self.text_bytes = (int(out[0]), int(out[1]))
        return self.text_bytes

    def download(self, mate: int = 0) -> np.ndarray:
        """Output `mate` of the block assembled last (uint8[])."""
        out = np.empty(self.text_bytes[mate], dtype=np.uint8)
        self._call("fqsx_fqtext_download", self._h, mate, out.ctypes.data if len(out) else None)
        return out

    def set_profiling(self, on: bool) -> None:
        self._lib.fqsx_fqtext_set_profiling(self._h, int(on))

    def kernel_times(self) -> dict:
        a = (C.c_double * 8)()
        self._lib.fqsx_fqtext_kernel_times(self._h, a)
        return {name: {"ms": a[k], "launches": int(a[4 + k])} for k, name in enumerate(FQTEXT_PASSES)}


class DeviceBlock:
    """A container block in device memory (DeviceColumns.block_dev): device pointers of its bases, its qualities and its
    offsets, valid until the next block is cut from the same columns, and the offsets on the host."""
    __slots__ = ("bases", "quals", "d_off", "off")

    def __init__(self, bases: int, quals: int, d_off: int, off: np.ndarray):
        self.bases, self.quals, self.d_off, self.off = bases, quals, d_off, off


class DeviceIds:
    """The id lines of a container block in device memory (DeviceColumns.ids_dev), the counterpart of DeviceBlock: device pointers
    of the lines and of their offsets, valid until the next id block is cut from the same columns, and the offsets on the host."""
    __slots__ = ("ids", "d_off", "off")

    def __init__(self, ids: int, d_off: int, off: np.ndarray):
        self.ids, self.d_off, self.off = ids, d_off, off


class DeviceColumns(_Handle):
    """The records of a FASTQ file with the base and the quality column resident in device memory (fqsx_cols_*), filled chunk by
    chunk by FastqParser.columns_into.  ids, id_off, read_off and plus_len are host arrays as in hostpipe.Columns, so that
    record_sizes(), ids_of / ids_of_pe and the block formation work as they do there; block_dev / block_pe_dev cut a block on
    the device where Columns.block / quals_of (block_pe / quals_of_pe) gather on the host.
    After keep_ids() the id column is resident too: `ids` stays empty (id_off as ever), ids_dev / ids_pe_dev cut a block's id
    lines on the device, and ids_of / ids_of_pe are that block downloaded."""
    keeps_ids = False

    def __init__(self, device: int = 0, lib_path: Optional[str] = None):
        from . import hostpipe as hp
        self._open(lib_path, "fqsx_cols_create", "fqsx_cols_destroy", device)
        self._set_host(hp.Columns.from_chunks([]))

    def keep_ids(self) -> None:
        """Before the first chunk: the store keeps the id column too (fqsx_cols_keep_ids).  FqsxError afterwards."""
        self._call("fqsx_cols_keep_ids", self._h)
        self.keeps_ids = True

    def _set_host(self, host) -> None:
        self._host = host
        self.ids, self.id_off, self.read_off, self.plus_len = host.ids, host.id_off, host.read_off, host.plus_len

    def set_host_columns(self, parts) -> None:
        """parts: what FastqParser.columns_into returned for every chunk appended to this store, in order"""
        from . import hostpipe as hp
        none = np.zeros(0, dtype=np.uint8)
        self._set_host(hp.Columns.from_chunks([(ids, id_off, none, read_off, none, read_off, plus_len) for ids, id_off, read_off, plus_len in parts]))

    def __len__(self) -> int:
        return len(self.read_off) - 1

    def record_sizes(self) -> np.ndarray:
        return self._host.record_sizes()

    def ids_of(self, idx):
        return self._ids_to_host(self.ids_dev(idx)) if self.keeps_ids else self._host.ids_of(idx)

    def ids_of_pe(self, mate2: "DeviceColumns", idx):
        return self._ids_to_host(self.ids_pe_dev(mate2, idx)) if self.keeps_ids else self._host.ids_of_pe(mate2._host, idx)

    def _ids_to_host(self, blk: DeviceIds):
        return self.download(blk.ids, int(blk.off[-1])), blk.off

    def gather_ids(self, idx, off: np.ndarray, mate2: Optional["DeviceColumns"] = None) -> DeviceIds:
        """fqsx_cols_gather_ids: the id lines of the reads idx (with mate2: of the pairs idx, mates interleaved) under the offsets off."""
        idx, off = self._gather_args(idx, off, mate2)
        out = [C.c_void_p() for _ in range(2)]
        self._call("fqsx_cols_gather_ids", self._h, mate2._h if mate2 is not None else None, idx.ctypes.data if len(idx) else None, len(idx),
                   off.ctypes.data, *[C.byref(p) for p in out])
        return DeviceIds(out[0].value, out[1].value, off)

    def ids_dev(self, idx) -> DeviceIds:
        idx = np.asarray(idx, dtype=np.int64)
        off = np.zeros(len(idx) + 1, dtype=np.uint64)
        io = self.id_off.view(np.int64)
        off[1:] = np.cumsum(io[idx + 1] - io[idx])
        return self.gather_ids(idx, off)

    def ids_pe_dev(self, mate2: "DeviceColumns", idx) -> DeviceIds:
        idx = np.asarray(idx, dtype=np.int64)
        ln = np.empty(2 * len(idx), dtype=np.int64)
        i1, i2 = self.id_off.view(np.int64), mate2.id_off.view(np.int64)
        ln[0::2], ln[1::2] = i1[idx + 1] - i1[idx], i2[idx + 1] - i2[idx]
        off = np.zeros(2 * len(idx) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(ln)
        return self.gather_ids(idx, off, mate2)

    def id_survey(self) -> dict:
        """fqsx_cols_id_survey: over the id lines of the store the four quantities the id kernel's staging limits are about."""
        a = (C.c_uint64 * 8)()
        self._call("fqsx_cols_id_survey", self._h, a)
        return {"keeps_ids": bool(a[0]), "id_bytes": int(a[1]), "max_line": int(a[2]), "max_tokens": int(a[3]), "max_name": int(a[4]),
                "max_name_tokens": int(a[5])}

    def info(self) -> dict:
        a, b = (C.c_uint64 * 4)(), (C.c_uint64 * 2)()
        self._call("fqsx_cols_info", self._h, a, fmt="{name}: {text}")
        self._call("fqsx_cols_id_info", self._h, b, fmt="{name}: {text}")
        return {"records": int(a[0]), "bases": int(a[1]), "device_bytes": int(a[2]), "device_bytes_peak": int(a[3]), "id_bytes": int(b[1])}

    @staticmethod
    def _gather_args(idx, off: np.ndarray, mate2):
        idx = np.asarray(idx)
        if len(idx) and (int(idx.min()) < 0 or int(idx.max()) >> 32):
            raise ValueError("read indices are 32-bit")
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        if len(off) != len(idx) * (2 if mate2 is not None else 1) + 1:
            raise ValueError("a block of n reads has n + 1 offsets")
        return idx, off

    def gather(self, idx, off: np.ndarray, mate2: Optional["DeviceColumns"] = None) -> DeviceBlock:
        """fqsx_cols_gather: the block of the reads idx (with mate2: of the pairs idx, mates interleaved) whose offsets are off."""
        idx, off = self._gather_args(idx, off, mate2)
        out = [C.c_void_p() for _ in range(3)]
        self._call("fqsx_cols_gather", self._h, mate2._h if mate2 is not None else None, idx.ctypes.data if len(idx) else None, len(idx),
                   off.ctypes.data, *[C.byref(p) for p in out])
        return DeviceBlock(out[0].value, out[1].value, out[2].value, off)

    def block_dev(self, idx) -> DeviceBlock:
        idx = np.asarray(idx, dtype=np.int64)
        off = np.zeros(len(idx) + 1, dtype=np.uint64)
        ro = self.read_off.view(np.int64)
        off[1:] = np.cumsum(ro[idx + 1] - ro[idx])
        return self.gather(idx, off)

    def block_pe_dev(self, mate2: "DeviceColumns", idx) -> DeviceBlock:
        idx = np.asarray(idx, dtype=np.int64)
        ln = np.empty(2 * len(idx), dtype=np.int64)
        r1, r2 = self.read_off.view(np.int64), mate2.read_off.view(np.int64)
        ln[0::2], ln[1::2] = r1[idx + 1] - r1[idx], r2[idx + 1] - r2[idx]
        off = np.zeros(2 * len(idx) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(ln)
        return self.gather(idx, off, mate2)

    def download(self, d_ptr: int, n_bytes: int) -> np.ndarray:
        """n_bytes of the store's device memory (a DeviceBlock's buffers) as a host array"""
        out = np.empty(n_bytes, dtype=np.uint8)
        self._call("fqsx_cols_download", self._h, d_ptr, out.ctypes.data, n_bytes)
        return out

    def sort_order(self, stats: Optional[dict] = None) -> List[np.ndarray]:
        """Read order of `fqs e -om s` for the store's records, sorted where they lie (fqsx_cols_sort_order): what sort_order
        returns for the same reads.  stats receives "passes" (radix passes) and "scratch_bytes" (device memory the call
        allocated at most, all of it handed back)."""
        order = np.empty(max(len(self), 1), dtype=np.uint32)
        bins = np.zeros(257, dtype=np.uint32)
        info = (C.c_uint64 * 4)()
        self._call("fqsx_cols_sort_order", self._h, order.ctypes.data, bins.ctypes.data, info)
        if stats is not None:
            stats["passes"], stats["scratch_bytes"] = int(info[0]), int(info[1])
        return _bins_of(order, bins)

    def bases_to_host(self) -> np.ndarray:
        """the whole base column"""
        out = np.empty(int(self.read_off[-1]), dtype=np.uint8)
        self._call("fqsx_cols_bases", self._h, out.ctypes.data)
        return out

    def set_profiling(self, on: bool) -> None:
        self._lib.fqsx_cols_set_profiling(self._h, int(on))

    def kernel_times(self) -> dict:
        a = (C.c_double * 4)()
        self._lib.fqsx_cols_kernel_times(self._h, a)
        b = (C.c_double * 6)()
        self._lib.fqsx_cols_id_kernel_times(self._h, b)
        return {"gather_ms": a[0], "gather_launches": int(a[1]), "check_ms": a[2], "check_launches": int(a[3]),
                "id_check_ms": b[0], "id_check_launches": int(b[1]), "id_gather_ms": b[2], "id_gather_launches": int(b[3]),
                "id_survey_ms": b[4], "id_survey_launches": int(b[5])}


def _chunk_source(src):
    """readinto-style reader over a path or over text already in memory (bytes / uint8 array)"""
    if isinstance(src, (str, os.PathLike)):
        f = open(src, "rb", buffering=0)
        return f.readinto, f.close
    data = np.frombuffer(src, dtype=np.uint8) if isinstance(src, (bytes, bytearray, memoryview)) else np.ascontiguousarray(src, dtype=np.uint8)
    pos = [0]

    def readinto(view) -> int:
        k = min(len(view), len(data) - pos[0])
        view[:k] = data[pos[0]:pos[0] + k]
        pos[0] += k
        return k
    return readinto, lambda: None


def bgzf_scan(data: np.ndarray, lib_path: Optional[str] = None, max_members: Optional[int] = None):
    """The BGZF members of `data` (uint8 array): (member_off, isize, bytes they span, bytes behind them, not_bgzf) --
    fqsx_bgzf_scan.  not_bgzf: what follows the members is no BGZF member header."""
    lib = load_library(lib_path)
    cap = len(data) // 28 + 1 if max_members is None else max_members   # (a member is 28 bytes at least)
    off, isize, out = np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint32), (C.c_uint64 * 4)()
    rc = lib.fqsx_bgzf_scan(data.ctypes.data if len(data) else None, len(data), cap, off.ctypes.data, isize.ctypes.data, out)
    if rc:
        raise _error(lib, "fqsx_bgzf_scan", rc, "bad argument")
    return off[:out[0]], isize[:out[0]], int(out[1]), int(out[2]), bool(out[3])


def bgzf_inflate(parser: FastqParser, members: np.ndarray, member_off: np.ndarray, text_bytes: int) -> np.ndarray:
    """The text of the BGZF members (as FastqParser.index_bgzf takes them; text_bytes: the sum of their ISIZE) inflated on the
    GPU and brought to the host -- fqsx_bgzf_inflate.  A damaged member: FqsxError with `.member` and `.kind`."""
    text, info = np.empty(text_bytes, dtype=np.uint8), (C.c_uint64 * 4)()
    member_off = np.ascontiguousarray(member_off, dtype=np.uint64)
    try:
        parser._call("fqsx_bgzf_inflate", parser._h, members.ctypes.data if len(members) else None, len(members),
                     member_off.ctypes.data if len(member_off) else None, len(member_off), text.ctypes.data, info)
    except FqsxError as e:
        if info[1]:
            e.member, e.kind = int(info[0]), INFLATE_KINDS[int(info[1])]
        raise
    return text


def _read_full(readinto, view) -> int:
    """fills view unless the source ends (a raw file may return fewer bytes than asked for)"""
    have = 0
    while have < len(view):
        k = readinto(view[have:])
        if not k:
            break
        have += k
    return have


def _sniffed(readinto, n: int = 2):
    """(the source's first n bytes, a readinto that begins with them again)"""
    head = bytearray(n)
    pending = [bytes(head[:_read_full(readinto, memoryview(head))])]

    def again(view) -> int:
        if pending[0]:
            k = min(len(view), len(pending[0]))
            view[:k] = pending[0][:k]
            pending[0] = pending[0][k:]
            return k
        return readinto(view)
    return pending[0], again


class _Gunzip:
    """readinto over the text of a gzip source (zlib on the host): member after member, so that concatenated gzip files -- BGZF
    among them -- read as one text.  ValueError: bytes behind the last member that are no gzip member, a source that ends inside one."""

    def __init__(self, readinto):
        self._src, self._buf, self._pend = readinto, bytearray(1 << 20), b""
        self._d, self._fresh, self._done = zlib.decompressobj(31), True, False
        self.members = self.compressed_bytes = 0

    def readinto(self, view) -> int:
        while not self._done:
            if not self._pend:
                k = self._src(memoryview(self._buf))
                if not k:
                    if not self._fresh:
                        raise ValueError("gzip input cut short inside member %d (after %d compressed bytes)" % (self.members, self.compressed_bytes))
                    self._done = True
                    break
                self._pend = bytes(self._buf[:k])
                self.compressed_bytes += k
            try:
                out = self._d.decompress(self._pend, len(view))
            except zlib.error as e:
                what = "bytes behind gzip member %d that are no gzip member" % (self.members - 1) if self._fresh and self.members else "damaged gzip member %d" % self.members
                raise ValueError("gzip input: %s (%s)" % (what, e)) from None
            self._fresh = False
            if self._d.eof:
                self.members += 1
                self._pend, self._d, self._fresh = self._d.unused_data, zlib.decompressobj(31), True
            else:
                self._pend = self._d.unconsumed_tail
            if out:
                view[:len(out)] = out
                return len(out)
        return 0


# What inflate="auto" does with a BGZF file: the GPU path, which tools/bgzf_inflate_bench.py measures against zlib on the host
# (profiles/bgzf_inflate.json)
BGZF_AUTO = "device"


def parse_fastq(text_or_path, device: int = 0, lib_path: Optional[str] = None, max_chunk_bytes: int = 0, stats: Optional[dict] = None,
                profile: bool = False, resident: bool = False, resident_ids: bool = False, inflate: str = "auto"):
    """FASTQ text (bytes / uint8 array) or a file (path) to hostpipe.Columns, parsed on the GPU chunk by chunk: a file is read in
    chunk-sized pieces into one reused buffer, the partial record at the end of a chunk is carried to the front of the next, and a
    chunk that holds no complete record doubles the chunk size.  What follows the last complete record (the reference drops an
    unterminated last record too) is not returned; its size is stats["tail_bytes"].  stats: also "chunks", "consumed",
    "max_id_line", "length_mismatch", "inflate" and -- profile -- "kernels".
    The input may be gzip, told by its first bytes (1f 8b), not by its name.  A BGZF file (bgzip) is inflated on the GPU, a
    chunk's worth of whole members at a time, straight into the buffer the parser reads: the compressed bytes are read in pieces,
    the partial member at the end of a piece is carried on the host and the partial record on the device, and no byte of the
    text comes to the host.  Any other gzip file -- several concatenated too -- is inflated by zlib on the host and parsed like
    text.  inflate: "device" (ValueError unless the file is BGZF), "host" (zlib for every gzip file) or "auto" (BGZF_AUTO for
    BGZF).  ValueError: a damaged BGZF member (its index, its offset in the file and the kind of damage), a file that ends inside
    a member, bytes behind the last member that are no member.  stats["inflate"]: "format" ("none", "gzip", "bgzf"), "where"
    ("host", "device"), "members", "compressed_bytes" and -- profile, on the device -- the kernel's "ms" and "launches".
    resident: a DeviceColumns instead -- the base and quality columns never come to the host (the caller closes it); ValueError
    for a record whose quality line differs in length from its base line, which resident columns cannot hold.
    resident_ids (with resident): the id column stays in device memory too (DeviceColumns.keep_ids): the store's `ids` is empty."""
    from . import hostpipe as hp
    if resident_ids and not resident:
        raise ValueError("resident_ids needs resident: the id column stays beside the two others")
    if inflate not in ("auto", "device", "host"):
        raise ValueError("inflate is 'auto', 'device' or 'host'")
    p = FastqParser(device, lib_path, max_chunk_bytes)
    store = DeviceColumns(device, lib_path) if resident else None
    readinto, close = _chunk_source(text_or_path)
    parts = []
    tot = {"chunks": 0, "consumed": 0, "max_id_line": 0, "length_mismatch": False}
    inf = {"format": "none", "where": "host", "members": 0, "compressed_bytes": 0}

    def take(info: dict) -> int:
        """the columns of the chunk indexed last; the bytes of it that its records are"""
        tot["chunks"] += 1
        if not info["records"]:
            return 0
        if resident and info["length_mismatch"]:
            raise LengthMismatch("a record's quality line differs in length from its base line: resident columns keep one offset array")
        parts.append(p.columns_into(info, store) if resident else p.columns(info))
        tot["max_id_line"] = max(tot["max_id_line"], info["max_id_line"])
        tot["length_mismatch"] |= info["length_mismatch"]
        tot["consumed"] += info["consumed"]
        return info["consumed"]

    def grown(size: int) -> int:
        if 2 * size >= 1 << 32:
            raise FqsxError("a FASTQ record of 2 GiB or more")
        return 2 * size

    def text_chunks(readinto) -> int:
        """chunks of text from the host; returns the bytes behind the last record"""
        size = p.max_chunk_bytes
        buf = np.empty(size, dtype=np.uint8)
        have, eof = 0, False
        while True:
            k = _read_full(readinto, memoryview(buf)[have:size]) if not eof else 0
            eof = eof or have + k < size
            have += k
            if have == 0:
                break
            used = take(p.index(buf[:have]))
            if used:
                buf[:have - used] = buf[used:have]   # the partial record goes to the front of the next chunk
                have -= used
            elif not eof:   # not one complete record in the chunk: a longer one
                size = grown(size)
                buf = np.concatenate([buf[:have], np.empty(size - have, dtype=np.uint8)])
            if eof:   # (the chunk held everything that was left: what it did not consume is no record)
                break
        return have

    def bgzf_chunks(readinto) -> int:
        """chunks of whole BGZF members, inflated on the device behind the partial record the chunk before left there"""
        limit = p.max_chunk_bytes                   # text per chunk
        piece = max(1 << 17, min(limit, 1 << 28) // 2)   # compressed bytes read at a time: two members at least
        buf = np.empty(piece, dtype=np.uint8)
        have, eof, base, carry = 0, False, 0, 0     # base: the file offset of buf[0]; carry: text kept on the device
        while True:
            if not eof:
                k = _read_full(readinto, memoryview(buf)[have:])
                eof = have + k < len(buf)
                have += k
                inf["compressed_bytes"] += k
            if have == 0:
                break
            off, isize, whole, _, not_bgzf = bgzf_scan(buf[:have], lib_path, max_members=min(have // 28 + 1, 1 << 20))
            if len(off) == 0:
                if not_bgzf:
                    raise ValueError("BGZF input: no BGZF member at offset %d (behind member %d)" % (base, inf["members"] - 1))
                if eof:
                    raise ValueError("BGZF input cut short inside member %d at offset %d" % (inf["members"], base))
                if have == len(buf):
                    raise ValueError("BGZF input: member %d at offset %d is longer than a member can be" % (inf["members"], base))
                continue
            n = max(1, int(np.searchsorted(carry + np.cumsum(isize.astype(np.int64)), limit, side="right")))
            span = int(off[n]) if n < len(off) else whole
            try:
                info = p.index_bgzf(buf[:span], off[:n], carry)
            except FqsxError as e:
                if getattr(e, "kind", None) is None:
                    raise
                raise ValueError("BGZF input: member %d at offset %d is damaged: %s" % (inf["members"] + e.member, base + int(off[e.member]), e.kind)) from None
            inf["members"] += n
            carry = info["text_bytes"] - take(info)
            if not info["records"] and carry >= limit:   # not one complete record in the chunk: a longer one
                limit = grown(limit)
            buf[:have - span] = buf[span:have]           # the partial member goes to the front of the next piece
            have -= span
            base += span
        return carry

    try:
        if resident_ids:
            store.keep_ids()
        p.set_profiling(profile)
        head, readinto = _sniffed(readinto)
        if head == b"\x1f\x8b":
            first, readinto = _sniffed(readinto, 1 << 16)   # (a BGZF header is 18 bytes unless it has further subfields)
            is_bgzf = len(bgzf_scan(np.frombuffer(first, dtype=np.uint8), lib_path, max_members=1)[0]) == 1
            if inflate == "device" and not is_bgzf:
                raise ValueError("inflate='device' needs BGZF input (bgzip): this gzip file's first member is none")
            inf["format"] = "bgzf" if is_bgzf else "gzip"
            inf["where"] = (BGZF_AUTO if inflate == "auto" else inflate) if is_bgzf else "host"
        if inf["where"] == "device":
            tail = bgzf_chunks(readinto)
            if profile:
                inf.update(p.inflate_times())
        elif inf["format"] != "none":
            gz = _Gunzip(readinto)
            tail = text_chunks(gz.readinto)
            inf.update(members=gz.members, compressed_bytes=gz.compressed_bytes)
        else:
            tail = text_chunks(readinto)
        if stats is not None:
            stats.update(tot, tail_bytes=tail, inflate=inf)
            if profile:
                stats["kernels"] = p.kernel_times()
    except BaseException:
        if store is not None:
            store.close()
        raise
    finally:
        close()
        p.close()
    if resident:
        store.set_host_columns(parts)
        return store
    return hp.Columns.from_chunks(parts)

