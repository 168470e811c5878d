"""One .fqs file's DNA path sharded over the GPUs of a node (BASELINE configs[3]).

Logical worker w of the T the bitstream fixes -- its coder state, RNG streams, local tables and the k-mer sub-tables it
owns (owner = function of the k-mer's prefix, fqs/dna.cpp:825; p-mers: index range, :658) -- lives on rank w % world,
one process per GPU.  Every rank holds a replica of all sub-tables for the look-ups.  One synchronisation phase of the
reference (the T x T mailboxes of fqs/application.h:56-59, applied by their owners in fqs/dna.cpp:2393-2472) runs inside
libfqsx.so (fqsx_shard_encode_block: one call per reads block) with three collectives and one host round trip:

    encode own workers, count what they pushed for whom
    all-reduce   [3][T][T] per-(source, owner) entry counts, [T] paired-end triples per source, one status word
                 -> every rank knows every transfer size and the tables' demand, and whether any rank's launch failed
    host round trip: the summed matrix, two demand words, the error word; buffers and tables grow here (a phase that
                 allocates or grows all-reduces one more word, the ranks' vote, before anything travels)
    all-to-all   the three mailboxes (u64 keys) in one grouped call -> keys reach their owner's rank in (source, push) order
    merge into the owners' groups, insert phase of own owners (their RNG streams stay here)
    all-gather   per rank: one (k-mer, final count) item per applied key of each kind, two words of p-mer vector
                 statistics, the paired-end triples of its sources -- with partitioned tables no s-/b-mer items but the
                 owners' occupancy counters -> replicas take the new slot values over, every rank inserts every pair
    clear the local tables

The transport is a C struct of three functions (include/fqsx.h: fqsx_comm):
  * RCCL inside the library, on the codec's own stream (fqsx_rccl_comm_create) -- the product path on MI355X;
  * callbacks into torch.distributed on buffers in host memory -- what the gloo tests run with the emulation build;
  * HBM buffers staged through the host (several ranks on one GPU: tests).
The per-worker streams are bit-identical to the one-GPU run's (tests/test_sharded_cpu.py), so the file a sharded run
writes is the same file.  With T <= 255 workers already concurrent on one GPU this mode cannot be faster than one GPU for
one file (DESIGN.md section 4 has the measured / counted overhead); replicas (bench.py --gpus N) remain the throughput mode.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch
import torch.distributed as dist

from .codec import DnaCodec, FqsxError


class _Comm(C.Structure):
    _AR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)
    _A2A = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64))
    _AG = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
    _AB = C.CFUNCTYPE(None, C.c_void_p)
    _fields_ = [("ctx", C.c_void_p), ("allreduce_sum_u32", _AR), ("alltoallv_u64", _A2A), ("allgather_u64", _AG), ("abort", _AB)]


def _host_tensor(addr: int, n: int, ctype, dtype) -> torch.Tensor:
    """n elements at a host address as a tensor that shares the memory"""
    return torch.from_numpy(np.ctypeslib.as_array((ctype * max(n, 1)).from_address(addr))[:n]).view(dtype)


def _torch_comm(world: int, group=None) -> _Comm:
    """fqsx_comm over torch.distributed for a codec whose memory space is host memory (the emulation build)."""
    def allreduce(_ctx, buf, n):
        try:
            dist.all_reduce(_host_tensor(buf, n, C.c_uint32, torch.int32), op=dist.ReduceOp.SUM, group=group)
            return 0
        except Exception as e:   # noqa: BLE001 -- reported through the C ABI
            print("fqsx transport:", e)
            return 1

    def alltoallv(_ctx, n_buf, send, scnt, recv, rcnt):
        try:
            for b in range(n_buf):
                n_out = [int(scnt[b * world + r]) for r in range(world)]
                n_in = [int(rcnt[b * world + r]) for r in range(world)]
                s = _host_tensor(send[b], sum(n_out), C.c_uint64, torch.int64)
                r = _host_tensor(recv[b], sum(n_in), C.c_uint64, torch.int64)
                dist.all_to_all_single(r, s, n_in, n_out, group=group)
            return 0
        except Exception as e:   # noqa: BLE001
            print("fqsx transport:", e)
            return 1

    def allgather(_ctx, send, n, recv):
        try:
            out = _host_tensor(recv, n * world, C.c_uint64, torch.int64)
            dist.all_gather_into_tensor(out, _host_tensor(send, n, C.c_uint64, torch.int64).clone(), group=group)
            return 0
        except Exception as e:   # noqa: BLE001
            print("fqsx transport:", e)
            return 1

    return _Comm(None, _Comm._AR(allreduce), _Comm._A2A(alltoallv), _Comm._AG(allgather))


def _staged_comm(world: int, group=None) -> _Comm:
    """fqsx_comm for a codec whose memory space is HBM when RCCL cannot carry the world -- several ranks on ONE device, which
    RCCL refuses (the two-process test of the partitioned tables on a one-GPU box): every collective is staged through host
    memory (hipMemcpy) and done by torch.distributed on the CPU (gloo).  A test and bring-up transport, not a fast one."""
    # (device buffers are wrapped as torch tensors in place: loading libamdhip64 a second time beside torch's own copy
    # would put two HIP runtimes into the process)
    class _Dev:
        def __init__(self, ptr, n, typestr):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}

    def dev(ptr, n, dtype):
        return torch.as_tensor(_Dev(ptr, n, "<i4" if dtype == torch.int32 else "<i8"), device="cuda")

    def down(ptr, n, dtype):
        return dev(ptr, n, dtype).cpu() if n else torch.empty(0, dtype=dtype)

    def up(ptr, t):
        if t.numel():
            dev(ptr, t.numel(), t.dtype).copy_(t)
            torch.cuda.synchronize()

    def guarded(f):
        def g(*a):
            try:
                torch.cuda.synchronize()   # (the codec's stream included: a device-wide wait)
                f(*a)
                return 0
            except Exception as e:   # noqa: BLE001 -- reported through the C ABI
                print("fqsx transport:", e)
                return 1
        return g

    @guarded
    def allreduce(_ctx, buf, n):
        t = down(buf, n, torch.int32)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        up(buf, t)

    @guarded
    def alltoallv(_ctx, n_buf, send, scnt, recv, rcnt):
        for b in range(n_buf):
            n_out = [int(scnt[b * world + r]) for r in range(world)]
            n_in = [int(rcnt[b * world + r]) for r in range(world)]
            r = torch.empty(max(sum(n_in), 1), dtype=torch.int64)[:sum(n_in)]
            dist.all_to_all_single(r, down(send[b], sum(n_out), torch.int64), n_in, n_out, group=group)
            up(recv[b], r)

    @guarded
    def allgather(_ctx, send, n, recv):
        out = torch.empty(n * world, dtype=torch.int64)
        dist.all_gather_into_tensor(out, down(send, n, torch.int64).clone(), group=group)
        up(recv, out)

    return _Comm(None, _Comm._AR(allreduce), _Comm._A2A(alltoallv), _Comm._AG(allgather))


class NativeShardedDnaCodec:
    """One file's DNA path over `world` ranks with the phase loop inside the library (fqsx_shard_encode_block).
    partition = True: the k-mer tables are partitioned over the ranks (fqsx_shard_partition_tables; one node).
    transport = "rccl": RCCL on the codec's stream; `id_bytes` = the 128-byte id rank 0 made with rccl_unique_id() and
    every rank received (e.g. through torch.distributed's store).  transport = "torch": torch.distributed collectives on
    host buffers (gloo; emulation build).  transport = "staged": HBM buffers staged through the host (see _staged_comm)."""

    def __init__(self, header: bytes, rank: int, world: int, device: int = 0, lib_path: Optional[str] = None, transport: str = "rccl",
                 id_bytes: Optional[bytes] = None, group=None, partition: bool = False, comm: Optional[_Comm] = None):
        self.codec = DnaCodec(header, device=device, lib_path=lib_path)
        self._lib, self._h, self.T = self.codec._lib, self.codec._h, self.codec.T
        self.rank, self.world, self.device = rank, world, device
        L = self._lib
        L.fqsx_shard_attach.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(_Comm)]
        L.fqsx_shard_encode_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.fqsx_shard_traffic.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.fqsx_rccl_comm_create.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(_Comm)]
        L.fqsx_rccl_comm_destroy.argtypes = [C.POINTER(_Comm)]
        self._rccl = transport == "rccl"
        self._staged = transport == "staged"
        self._own_comm = True
        if self._rccl and comm is not None:   # the process's communicator, made with an earlier codec: goes on with this one's stream
            L.fqsx_rccl_comm_rebind.argtypes = [C.POINTER(_Comm), C.c_void_p]
            self._comm, self._own_comm = comm, False
            self._ck(L.fqsx_rccl_comm_rebind(C.byref(self._comm), self._h), "fqsx_rccl_comm_rebind")
        elif self._rccl:
            if id_bytes is None or len(id_bytes) != 128:
                raise ValueError("the RCCL transport needs the 128-byte unique id (rccl_unique_id on rank 0)")
            self._comm = _Comm()
            self._ck(L.fqsx_rccl_comm_create(self._h, bytes(id_bytes), rank, world, C.byref(self._comm)), "fqsx_rccl_comm_create")
        elif transport == "staged":
            self._comm = _staged_comm(world, group)
        else:
            self._comm = comm if comm is not None else _torch_comm(world, group)
        self._ck(L.fqsx_shard_attach(self._h, rank, world, C.byref(self._comm)), "fqsx_shard_attach")
        self.partitioned = False
        self.partition_note = ""
        if partition:   # (collective) each rank keeps 1/world of the k-mer tables and maps the rest from its peers
            L.fqsx_shard_partition_tables.argtypes = [C.c_void_p]
            L.fqsx_shard_is_partitioned.argtypes = [C.c_void_p]
            self._ck(L.fqsx_shard_partition_tables(self._h), "fqsx_shard_partition_tables")
            self.partitioned = bool(L.fqsx_shard_is_partitioned(self._h))
            if not self.partitioned:   # GPUs without peer access: the whole world stays with replicas (same streams)
                self.partition_note = self._lib.fqsx_last_error().decode()
                if rank == 0:
                    import warnings
                    warnings.warn("fqsx: " + self.partition_note)
        self.own_workers = list(range(rank, self.T, world))
        self._streams = (C.c_void_p * self.T)()
        self._lens = (C.c_uint64 * self.T)()

    @staticmethod
    def rccl_unique_id(lib_path: Optional[str] = None) -> bytes:
        from .codec import load_library
        lib = load_library(lib_path)
        buf = C.create_string_buffer(128)
        lib.fqsx_rccl_unique_id.argtypes = [C.c_char_p]
        if lib.fqsx_rccl_unique_id(buf):
            raise FqsxError(f"fqsx_rccl_unique_id: {lib.fqsx_last_error().decode()}")
        return buf.raw

    def _ck(self, rc: int, what: str) -> None:
        if rc:
            raise FqsxError(f"{what}: {rc}: {self._lib.fqsx_last_error().decode()}")

    def encode_block(self, bases: np.ndarray, read_off: np.ndarray, generation: int) -> Dict[int, bytes]:
        """All ranks call this with the same block; returns {worker: DNA stream} for this rank's workers."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        if self._rccl or self._staged:   # the codec's memory space is HBM
            dev = torch.device("cuda", self.device)
            t_b, t_o = torch.from_numpy(bases).to(dev), torch.from_numpy(read_off.view(np.int64)).to(dev)
            torch.cuda.synchronize(dev)
            pb, po = t_b.data_ptr(), t_o.data_ptr()
        else:
            pb, po = bases.ctypes.data, read_off.ctypes.data
        self._ck(self._lib.fqsx_shard_encode_block(self._h, pb, po, read_off.ctypes.data, len(read_off) - 1, generation, self._streams, self._lens),
                 "fqsx_shard_encode_block")
        return {w: (C.string_at(self._streams[w], self._lens[w]) if self._lens[w] else b"") for w in self.own_workers}

    def encode_block_dev(self, d_bases_ptr: int, d_off_ptr: int, read_off: np.ndarray, generation: int) -> int:
        """block already in HBM; returns the bytes of this rank's streams"""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        self._ck(self._lib.fqsx_shard_encode_block(self._h, d_bases_ptr, d_off_ptr, read_off.ctypes.data, len(read_off) - 1, generation, self._streams, self._lens),
                 "fqsx_shard_encode_block")
        return sum(self._lens[w] for w in self.own_workers)

    @property
    def traffic(self) -> dict:
        a = (C.c_uint64 * 4)()
        self._lib.fqsx_shard_traffic(self._h, a)
        return {"phases": a[0], "collectives": a[1], "all_to_all_bytes": 8 * a[2], "all_gather_bytes": 8 * a[3]}

    def rccl_info(self) -> dict:
        """what RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank)"""
        a = (C.c_uint32 * 2)()
        self._lib.fqsx_rccl_comm_info.argtypes = [C.POINTER(_Comm), C.POINTER(C.c_uint32)]
        self._ck(self._lib.fqsx_rccl_comm_info(C.byref(self._comm), a), "fqsx_rccl_comm_info")
        return {"ranks_seen": int(a[0]), "rank": int(a[1])}

    def detach_comm(self) -> "_Comm":
        """keep the RCCL communicator beyond this codec (hand it to the next NativeShardedDnaCodec as `comm`)"""
        self._own_comm = False
        return self._comm

    def destroy_comm(self) -> None:
        if self._rccl and self._comm.ctx:
            self._lib.fqsx_rccl_comm_destroy(C.byref(self._comm))

    def close(self) -> None:
        if self._rccl and self._own_comm and self._comm.ctx:
            self._lib.fqsx_rccl_comm_destroy(C.byref(self._comm))
        self.codec.close()
