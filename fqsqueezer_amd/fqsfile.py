"""Write a complete `.fqs` file around the GPU streams, readable by the reference decompressor `fqs d` and
byte-identical to what `fqs e -t <threads>` writes for the same input and modes.  Host plumbing: block
formation, worker offsets, the container, the meta and id streams (host C++ helpers,
csrc/fqsx_host.cpp); the DNA and quality streams come from the GPU (codec.DnaCodec / codec.QualCodec)."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import hostpipe as hp
from .codec import DeviceBlock, DnaCodec, FqsxError, IdCodec, MetaCodec, QualCodec, parse_fastq, sort_order


def _gpu_groups(rec: hp.Records, device: int, lib_path: Optional[str]):
    """Sorted-mode read order from the GPU pre-pass (bins + per-bin order incl. the reference's order of equal reads)."""
    bases, off = hp.block_arrays(rec, np.arange(len(rec), dtype=np.int64))
    return sort_order(bases, off, device=device, lib_path=lib_path)


class _Ids:
    """The id coder of one file: the GPU kernel, or -- once the kernel reports an id beyond its staging limits or its list of
    instrument names (IdCodec.encode_block, `staging`) -- the host coder, brought to the same state by coding again the id
    columns of the blocks written so far (of which only the index arrays are kept; ids_of(idx) cuts the columns again).  The
    blocks already written stay as they are: both coders write the same bytes.  The encoder's twin of fqsread._Ids."""

    def __init__(self, header: bytes, device: int, lib_path: Optional[str], gpu_ids: bool, paired: bool, ids_of):
        self.header, self.lib_path, self.paired, self.ids_of = header, lib_path, paired, ids_of
        self.enc = IdCodec(header, lib_path=lib_path, device=device if gpu_ids else None)
        self.on_gpu = gpu_ids
        self.seen = []   # the index arrays of the blocks coded on the GPU so far
        self.fell_back = False

    def encode(self, idx, ids, id_off):
        if self.on_gpu:
            try:
                out = self.enc.encode_block(ids, id_off, self.paired)
                self.seen.append(idx)
                return out
            except FqsxError as e:
                if not getattr(e, "staging", False):
                    raise
            self.enc.close()
            self.enc = IdCodec(self.header, lib_path=self.lib_path)
            self.on_gpu, self.fell_back = False, True
            for j in self.seen:
                self.enc.encode_block(*self.ids_of(j), self.paired)
            self.seen = []
        return self.enc.encode_block(ids, id_off, self.paired)

    def close(self):
        self.enc.close()


def encode_blocks(header: bytes, blocks, arrays, sizes_of, paired: bool, device: int, lib_path: Optional[str], stats: Optional[dict] = None,
                  gpu_ids: bool = True, ids_of=None):
    """Generator of the file's container blocks.  Per block the four coders run side by side, as the reference's worker
    codes meta, id, DNA and quality of a read in one loop (application.cpp:633-641): the DNA kernels and the quality kernel
    and the id kernel on their own HIP streams (host threads inside the C ABI, which releases the GIL), the meta coder on a host
    thread meanwhile.  arrays(idx) may hand back the bases as a codec.DeviceBlock (a block cut on the device, its qualities with
    it): the DNA and quality coders then read it where it lies.  ids_of(idx): the id columns of a block alone (default: from
    arrays), for the id coder's change-over to the host coder in mid-file (_Ids); stats then has "id_host_fallback" True."""
    from concurrent.futures import ThreadPoolExecutor
    threads = header[4]
    stored = hp.stored_streams(header)
    dna = DnaCodec(header, device=device, lib_path=lib_path)
    meta = MetaCodec(threads, lib_path=lib_path)
    # (the id stream comes from the GPU coder too: fqsx_idg_*, one wavefront per worker on a stream of its own; gpu_ids = False:
    # the host coder, one host thread per worker -- the same bytes)
    idc = _Ids(header, device, lib_path, gpu_ids, paired, ids_of or (lambda idx: arrays(idx)[2:4])) if hp.STREAM_ID in stored else None
    qual = QualCodec(header, device=device, lib_path=lib_path) if hp.STREAM_QUALITY in stored else None
    pool = ThreadPoolExecutor(max_workers=3)
    try:
        for g, idx in enumerate(blocks):
            bases, off, ids, id_off, quals = arrays(idx)
            n = len(off) - 1
            if isinstance(bases, DeviceBlock):
                jobs = {hp.STREAM_DNA: pool.submit(dna.encode_block_dev, bases.bases, bases.d_off, off, g)}
                if qual is not None:
                    jobs[hp.STREAM_QUALITY] = pool.submit(qual.encode_block_dev, bases.quals, bases.d_off, off, True)
            else:
                jobs = {hp.STREAM_DNA: pool.submit(dna.encode_block, bases, off, g)}
                if qual is not None:
                    jobs[hp.STREAM_QUALITY] = pool.submit(qual.encode_block, quals, off)
            if idc is not None:
                jobs[hp.STREAM_ID] = pool.submit(idc.encode, idx, ids, id_off)
            st = {hp.STREAM_META: meta.encode_block(np.diff(off.astype(np.int64)).astype(np.uint32), paired)}
            for k, f in jobs.items():
                st[k] = f.result()
            cs = np.concatenate([[0], np.cumsum(sizes_of(idx))])
            blk = hp.FqsBlock(n)
            for w, (first, _) in enumerate(hp.partition_for_workers(n, threads)):
                blk.offsets.append(int(cs[first]) if n else 0)   # application.cpp:716
                blk.streams.append({k: v[w] for k, v in st.items()})
            yield blk
        if stats is not None:
            stats["dna"] = dna.stats()
            stats["dna_capacity"] = dna.capacity()
            stats["id_host_fallback"] = idc is not None and idc.fell_back
            try:   # everything this process holds on the device at the end of the file: DNA tables + quality models + id models + block buffers
                import torch
                free, total = torch.cuda.mem_get_info(device)
                stats["device_bytes_in_use"] = int(total - free)
            except Exception:   # noqa: BLE001 -- extra information only
                pass
    finally:
        pool.shutdown(wait=True)
        dna.close()
        meta.close()
        if idc is not None:
            idc.close()
        if qual is not None:
            qual.close()


def _encode(header: bytes, blocks, arrays, sizes_of, paired: bool, device: int, lib_path: Optional[str], gpu_ids: bool = True,
            stats: Optional[dict] = None, ids_of=None) -> bytes:
    return hp.write_fqs(header, encode_blocks(header, blocks, arrays, sizes_of, paired, device, lib_path, stats=stats, gpu_ids=gpu_ids, ids_of=ids_of))


# What the id kernel stages of an id line in LDS, the one place on this side that states csrc/fqsx_idk.h's IDK_MAX_ID, IDK_MAX_TOK
# and IDK_NAME - 2: a line of at most 1024 bytes with its line feed, at most 128 tokens, an instrument name of at most 62 bytes
_ID_LINE_MAX, _ID_TOKENS_MAX, _ID_NAME_MAX = 1024, 128, 62
_ID_LITERAL = np.zeros(256, dtype=bool)   # idk_is_lit (id.cpp:57-70): every other byte ends a token, the line feed included
_ID_LITERAL[list(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz@")] = True
_ID_NAME_END = np.zeros(256, dtype=bool)
_ID_NAME_END[list(b". :")] = True


def _first_at_or_after(marks: np.ndarray, start: np.ndarray, stop: np.ndarray) -> np.ndarray:
    """per line [start, stop): the position of its first marked byte, stop if it has none (marks: sorted positions)"""
    if not len(marks):
        return stop.copy()
    k = np.searchsorted(marks, start)
    at = marks[np.minimum(k, len(marks) - 1)]
    return np.where((k < len(marks)) & (at < stop), at, stop)


def _id_lines_fit_the_kernel(ids: np.ndarray, id_off: np.ndarray, id_mode: str) -> bool:
    """The id kernel's rule (idk_id_lossless / idk_id_instrument / idk_lossless, csrc/fqsx_idk.h) for the id lines `ids` (each
    with its line feed), in one pass: False if the kernel would answer one of them with IDK_ERR_TOO_LONG.  Lossless mode: the
    line with its line feed within _ID_LINE_MAX bytes and within _ID_TOKENS_MAX tokens.  Instrument mode: the line within
    _ID_LINE_MAX; the name -- up to the first '.', ' ' or ':', cut short at a NUL -- within _ID_NAME_MAX bytes; and, as a new
    name is coded through the lossless path with a terminating NUL, the bytes up to the '.', ' ' or ':' within _ID_TOKENS_MAX
    tokens with that terminator.  (A line without a name, or with a byte >= 128 where it is coded, is refused by both coders: not a
    staging matter.)"""
    off = np.asarray(id_off).astype(np.int64)
    if len(off) < 2:
        return True
    start, stop = off[:-1], off[1:]
    if int((stop - start).max()) > _ID_LINE_MAX:
        return False
    ids = np.asarray(ids)
    seps = np.zeros(len(ids) + 1, dtype=np.int64)
    np.cumsum(~_ID_LITERAL[ids], out=seps[1:])
    if id_mode != "instrument":
        return int((seps[stop] - seps[start]).max()) <= _ID_TOKENS_MAX
    end = _first_at_or_after(np.flatnonzero(_ID_NAME_END[ids]), start, stop)
    named = end < stop
    name_len = _first_at_or_after(np.flatnonzero(ids == 0), start, end) - start
    return not bool((named & ((name_len > _ID_NAME_MAX) | (seps[end] - seps[start] + 1 > _ID_TOKENS_MAX))).any())


def _ids_fit_the_kernel(id_mode: str, *recs) -> bool:
    """False if an id of the file is beyond what the GPU id coder stages (the host coder, like the reference, has no limits):
    a cheap pre-scan so that the file goes to the host coder as a whole instead of changing over in mid-file.  (What no
    pre-scan of lines can know, the number of different instrument names a worker meets, is left to that change-over.)"""
    return all(_id_lines_fit_the_kernel(*hp.id_arrays(rec, np.arange(len(rec))), id_mode) for rec in recs)


def compress_records(rec: hp.Records, threads: int, order: str = "s", genome_size_mbp: int = 3100, device: int = 0,
                     lib_path: Optional[str] = None, quality_mode: str = "none", id_mode: str = "none",
                     quality_thr: int = 20, as_blocks: bool = False, gpu_ids: Optional[bool] = None, stats: Optional[dict] = None):
    """`fqs e -s -om <order> -t <threads> -gs <g> -qm <..> -im <..>` on single-end records.  Returns the file's bytes, or
    -- as_blocks -- (header, generator of container blocks) for files too large to hold (hostpipe.fqs_chunks serialises them).
    gpu_ids: the id stream from the GPU kernel (True), from the host coder (False: one thread per worker, no limits on the id
    lines), or -- None -- the kernel unless an id of the file is beyond its staging limits.  A file on the kernel that meets
    more instrument names than a worker's list holds goes on with the host coder from that block (the same bytes).  stats:
    "gpu_ids" (the choice made), "id_host_fallback" (changed over in mid-file) and what encode_blocks adds."""
    if gpu_ids is None:
        gpu_ids = id_mode == "none" or _ids_fit_the_kernel(id_mode, rec)
    if stats is not None:
        stats["gpu_ids"] = gpu_ids
    mode = "se_sorted" if order == "s" else "se_original"
    header = hp.make_header(threads, mode, genome_size_mbp, quality_mode, id_mode, quality_thr)
    sizes = rec.record_sizes()

    def ids_of(idx):
        return hp.id_arrays(rec, idx)

    def arrays(idx):
        bases, off = hp.block_arrays(rec, idx)
        ids, id_off = ids_of(idx) if id_mode != "none" else (None, None)
        quals = hp.qual_arrays(rec, idx)[0] if quality_mode != "none" else None
        return bases, off, ids, id_off, quals

    groups = _gpu_groups(rec, device, lib_path) if mode == "se_sorted" else None
    if as_blocks:
        return header, encode_blocks(header, hp.form_blocks(rec, mode, groups=groups), arrays, lambda idx: sizes[idx], False, device, lib_path, stats=stats,
                                     gpu_ids=gpu_ids, ids_of=ids_of)
    return _encode(header, hp.form_blocks(rec, mode, groups=groups), arrays, lambda idx: sizes[idx], False, device, lib_path, gpu_ids, stats, ids_of)


def compress_records_pe(rec1: hp.Records, rec2: hp.Records, threads: int, order: str = "s", genome_size_mbp: int = 3100,
                        device: int = 0, lib_path: Optional[str] = None, quality_mode: str = "none", id_mode: str = "none",
                        quality_thr: int = 20, as_blocks: bool = False, gpu_ids: Optional[bool] = None, stats: Optional[dict] = None):
    """`fqs e -p ...` on two mate files (records interleaved mate 1 / mate 2 inside a block).  gpu_ids: see compress_records."""
    if gpu_ids is None:
        gpu_ids = id_mode == "none" or _ids_fit_the_kernel(id_mode, rec1, rec2)
    if stats is not None:
        stats["gpu_ids"] = gpu_ids
    mode = "pe_sorted" if order == "s" else "pe_original"
    header = hp.make_header(threads, mode, genome_size_mbp, quality_mode, id_mode, quality_thr)
    s1, s2 = rec1.record_sizes(), rec2.record_sizes()

    def ids_of(idx):
        return hp.id_arrays_pe(rec1, rec2, idx)

    def arrays(idx):
        bases, off = hp.block_arrays_pe(rec1, rec2, idx)
        ids, id_off = ids_of(idx) if id_mode != "none" else (None, None)
        quals = hp.qual_arrays_pe(rec1, rec2, idx)[0] if quality_mode != "none" else None
        return bases, off, ids, id_off, quals

    def sizes_of(idx):
        z = np.empty(2 * len(idx), dtype=np.int64)
        z[0::2], z[1::2] = s1[idx], s2[idx]
        return z

    groups = _gpu_groups(rec1, device, lib_path) if mode == "pe_sorted" else None   # mates follow mate 1's order, io.h:541-550
    if as_blocks:
        return header, encode_blocks(header, hp.form_blocks_pe(rec1, rec2, mode, groups=groups), arrays, sizes_of, True, device, lib_path, stats=stats,
                                     gpu_ids=gpu_ids, ids_of=ids_of)
    return _encode(header, hp.form_blocks_pe(rec1, rec2, mode, groups=groups), arrays, sizes_of, True, device, lib_path, gpu_ids, stats, ids_of)


def _id_columns_fit_the_kernel(cols: hp.Columns, max_id_line: int, id_mode: str) -> bool:
    """_ids_fit_the_kernel on columns: the parser's longest id line (it counts the line feed) and one pass over the id bytes."""
    return max_id_line <= _ID_LINE_MAX and _id_lines_fit_the_kernel(cols.ids, cols.id_off.view(np.int64), id_mode)


def compress_fastq(text_or_path, text2_or_path2=None, threads: int = 1, order: str = "s", genome_size_mbp: int = 3100,
                   quality_mode: str = "illumina_8", id_mode: str = "instrument", quality_thr: int = 20, device: int = 0,
                   lib_path: Optional[str] = None, as_blocks: bool = False, gpu_ids: Optional[bool] = None, stats: Optional[dict] = None,
                   max_chunk_bytes: int = 0, resident: bool = False, profile: bool = False):
    """`fqs e` on FASTQ files: `-s` with one input, `-p` with two (text as bytes / uint8 array, or a path; the defaults are the
    reference's, params.h:53-78).  The text is parsed on the GPU into columns (codec.parse_fastq), the sort pre-pass runs on the
    base column, and the blocks are cut from the columns with vectorised gathers.  Returns what compress_records* return.
    ValueError: a record whose quality line differs in length from its base line; mate files with different numbers of records.
    gpu_ids: see compress_records.  stats: "parse" (one dict per input), "gpu_ids" (the choice made), "id_host_fallback" (the id coder
    changed over to the host coder in mid-file) and what encode_blocks adds.
    resident: the base and quality columns stay in device memory (codec.DeviceColumns, one store per input) and the blocks are
    cut there; the same bytes.  Sorted order brings the base column to the host once, for the sort pre-pass; qualities never
    come to the host.  stats then also has "columns" (DeviceColumns.info() per input once the last block is written, with
    -- profile -- the gather kernel's "kernels")."""
    paired = text2_or_path2 is not None
    cols, parse_stats = [], []
    try:
        for src in (text_or_path, text2_or_path2)[:2 if paired else 1]:
            st = {}
            try:
                cols.append(parse_fastq(src, device=device, lib_path=lib_path, max_chunk_bytes=max_chunk_bytes, stats=st, resident=resident))
            except ValueError:   # (resident columns cannot hold such a record: parse_fastq stops at its chunk)
                st["length_mismatch"] = True
            parse_stats.append(st)
            if st["length_mismatch"]:
                raise ValueError("a record's quality line differs in length from its base line (input %d)" % len(parse_stats))
        out = _compress_columns(cols, parse_stats, threads, order, genome_size_mbp, quality_mode, id_mode, quality_thr, device, lib_path, gpu_ids,
                                stats, resident, profile)
    except BaseException:
        if resident:
            for c in cols:
                c.close()
        raise
    return out if as_blocks else hp.write_fqs(*out)


def _closing_columns(gen, cols, stats: Optional[dict], profile: bool):
    """the blocks of gen; then the device columns are released"""
    try:
        yield from gen
        if stats is not None:
            stats["columns"] = [dict(c.info(), **({"kernels": c.kernel_times()} if profile else {})) for c in cols]
    finally:
        for c in cols:
            c.close()


def _compress_columns(cols, parse_stats, threads, order, genome_size_mbp, quality_mode, id_mode, quality_thr, device, lib_path, gpu_ids,
                      stats, resident, profile):
    """(header, generator of container blocks) from the parsed columns of compress_fastq's one or two inputs"""
    paired = len(cols) == 2
    if paired and len(cols[0]) != len(cols[1]):
        raise ValueError("the mate files hold different numbers of records: %d and %d" % (len(cols[0]), len(cols[1])))
    if gpu_ids is None:
        gpu_ids = id_mode == "none" or all(_id_columns_fit_the_kernel(c, st["max_id_line"], id_mode) for c, st in zip(cols, parse_stats))
    if stats is not None:
        stats["parse"], stats["gpu_ids"] = parse_stats, gpu_ids
    mode = ("pe_" if paired else "se_") + ("sorted" if order == "s" else "original")
    header = hp.make_header(threads, mode, genome_size_mbp, quality_mode, id_mode, quality_thr)
    c1 = cols[0]
    # mates follow mate 1's order
    groups = sort_order(c1.bases_to_host() if resident else c1.bases, c1.read_off, device=device, lib_path=lib_path) if order == "s" else None
    if resident and profile:
        c1.set_profiling(True)
    if paired:
        c2 = cols[1]
        s1, s2 = c1.record_sizes(), c2.record_sizes()

        def ids_of(idx):
            return c1.ids_of_pe(c2, idx)

        def arrays(idx):
            ids, id_off = ids_of(idx) if id_mode != "none" else (None, None)
            if resident:
                blk = c1.block_pe_dev(c2, idx)
                return blk, blk.off, ids, id_off, None
            bases, off = c1.block_pe(c2, idx)
            quals = c1.quals_of_pe(c2, idx)[0] if quality_mode != "none" else None
            return bases, off, ids, id_off, quals

        def sizes_of(idx):
            z = np.empty(2 * len(idx), dtype=np.int64)
            z[0::2], z[1::2] = s1[idx], s2[idx]
            return z

        blocks = hp.form_blocks_pe(c1, c2, mode, groups=groups)
    else:
        sizes = c1.record_sizes()

        def ids_of(idx):
            return c1.ids_of(idx)

        def arrays(idx):
            ids, id_off = ids_of(idx) if id_mode != "none" else (None, None)
            if resident:
                blk = c1.block_dev(idx)
                return blk, blk.off, ids, id_off, None
            bases, off = c1.block(idx)
            quals = c1.quals_of(idx)[0] if quality_mode != "none" else None
            return bases, off, ids, id_off, quals

        def sizes_of(idx):
            return sizes[idx]

        blocks = hp.form_blocks(c1, mode, groups=groups)
    gen = encode_blocks(header, blocks, arrays, sizes_of, paired, device, lib_path, stats=stats, gpu_ids=gpu_ids, ids_of=ids_of)
    return header, (_closing_columns(gen, cols, stats, profile) if resident else gen)


_QM = {"o": "lossless", "8": "illumina_8", "4": "illumina_4", "2": "binary", "n": "none"}   # fqsqueezer.cpp:157-191
_IM = {"o": "lossless", "i": "instrument", "n": "none"}


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m fqsqueezer_amd.fqsfile", description="compress FASTQ files to a .fqs file on the GPU (`fqs e`)")
    ap.add_argument("cmd", choices=["e"])
    ends = ap.add_mutually_exclusive_group()
    ends.add_argument("-s", dest="paired", action="store_false", help="single-end: one input file (default)")
    ends.add_argument("-p", dest="paired", action="store_true", help="paired-end: two input files")
    ap.add_argument("-t", type=int, default=1, help="worker threads of the bitstream, 1..64")
    ap.add_argument("-gs", type=int, default=3100, help="genome size in Mbp, 1..32768")
    ap.add_argument("-om", choices=["o", "s"], default="s", help="read order: original / sorted")
    ap.add_argument("-qm", choices=list(_QM), default="8", help="quality mode")
    ap.add_argument("-qt", type=int, default=20, help="quality threshold of -qm 2")
    ap.add_argument("-im", choices=list(_IM), default="i", help="id mode")
    ap.add_argument("-out", default="output.fqs")
    ap.add_argument("-device", type=int, default=0)
    ap.add_argument("-lib", default=None, help="path of the library to load (default: the package's libfqsx.so)")
    ap.add_argument("-resident", action="store_true", help="keep the base and quality columns in device memory and cut the blocks there")
    ap.add_argument("inputs", nargs="+")
    a = ap.parse_args(argv)
    if len(a.inputs) != (2 if a.paired else 1):
        ap.error("-p takes two input files, -s one")
    header, blocks = compress_fastq(a.inputs[0], a.inputs[1] if a.paired else None, threads=min(max(a.t, 1), 64), order=a.om,
                                    genome_size_mbp=min(max(a.gs, 1), 32768), quality_mode=_QM[a.qm], id_mode=_IM[a.im], quality_thr=a.qt,
                                    device=a.device, lib_path=a.lib, as_blocks=True, resident=a.resident)
    with open(a.out, "wb") as f:
        for chunk in hp.fqs_chunks(header, blocks):   # block by block: the file is never held whole
            f.write(chunk)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
