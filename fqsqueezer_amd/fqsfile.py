"""Write a complete `.fqs` file around the GPU streams, readable by the reference decompressor `fqs d` and
byte-identical to what `fqs e -t <threads>` writes for the same input and modes.  Host plumbing: block
formation, worker offsets, the container, the meta and id streams (host C++ helpers,
csrc/fqsx_host.cpp); the DNA and quality streams come from the GPU (codec.DnaCodec / codec.QualCodec)."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import hostpipe as hp
from .codec import DeviceBlock, DeviceColumns, DeviceIds, DnaCodec, IdFallback, LengthMismatch, MetaCodec, QualCodec, parse_fastq, sort_order


def _gpu_groups(rec, device: int, lib_path: Optional[str], stats: Optional[dict] = None):
    """Sorted-mode read order from the GPU pre-pass (bins + per-bin order incl. the reference's order of equal reads) on the base
    column of rec: hostpipe.Records, hostpipe.Columns or codec.DeviceColumns (sorted in the store: no base comes to the host).
    stats["sort"]: "resident", "passes" and "scratch_bytes" of the store's sort, or "resident" False and "batches"."""
    st = {"resident": isinstance(rec, DeviceColumns)}
    if st["resident"]:
        groups = rec.sort_order(stats=st)
    else:
        bases, off = rec.block(np.arange(len(rec), dtype=np.int64)) if isinstance(rec, hp.Records) else (rec.bases, rec.read_off)
        groups = sort_order(bases, off, device=device, lib_path=lib_path, stats=st)
    if stats is not None:
        stats["sort"] = st
    return groups


def encode_blocks(header: bytes, blocks, arrays, sizes_of, paired: bool, device: int, lib_path: Optional[str], stats: Optional[dict] = None,
                  gpu_ids: bool = True, ids_of=None):
    """Generator of the file's container blocks.  Per block the four coders run side by side, as the reference's worker
    codes meta, id, DNA and quality of a read in one loop (application.cpp:633-641): the DNA kernels and the quality kernel
    and the id kernel on their own HIP streams (host threads inside the C ABI, which releases the GIL), the meta coder on a host
    thread meanwhile.  arrays(idx) may hand back the bases as a codec.DeviceBlock (a block cut on the device, its qualities with
    it): the DNA and quality coders then read it where it lies.  ids_of(idx): the id columns of a block alone (default: from
    arrays), for the id coder's change-over to the host coder in mid-file (codec.IdFallback); stats then has "id_host_fallback" True.
    arrays(idx) may also hand back the ids as a codec.DeviceIds (id lines cut on the device), which the id kernel reads where they
    lie, or as None: the id job then cuts them itself with ids_of(idx) -- from its own thread, while this one waits for it and
    touches no column store."""
    from concurrent.futures import ThreadPoolExecutor
    threads = header[4]
    stored = hp.stored_streams(header)
    dna = DnaCodec(header, device=device, lib_path=lib_path)
    meta = MetaCodec(threads, lib_path=lib_path)
    # (the id stream comes from the GPU coder too: fqsx_idg_*, one wavefront per worker on a stream of its own; gpu_ids = False:
    # the host coder, one host thread per worker -- the same bytes)
    # of a block coded on the kernel only the index array is kept: a change-over to the host coder in mid-file (codec.IdFallback)
    # cuts its id columns again; a block's first run takes the columns arrays(idx) has cut already
    ids_of = ids_of or (lambda idx: arrays(idx)[2:4])

    def code_ids(enc, idx, held):
        """held: (DeviceIds, its offsets) for the kernel coder -- the host coder, after a change-over, cuts the block again as it cuts
        the blocks before it --, (ids, id_off) host arrays, or None"""
        if held is not None and isinstance(held[0], DeviceIds):
            if enc.on_device:
                return enc.encode_block_dev(held[0].ids, held[0].d_off, held[0].off, paired)
            held = None
        return enc.encode_block(*(held or ids_of(idx)), paired)
    idc = IdFallback(header, device, lib_path, gpu_ids, code_ids) if hp.STREAM_ID in stored else None
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
                jobs[hp.STREAM_ID] = pool.submit(idc.run, idx, (ids, id_off) if ids is not None else None)
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


def _id_maxima_fit(id_mode: str, max_line: int, max_tokens: int, max_name: int, max_name_tokens: int) -> bool:
    """The id kernel's rule (idk_id_lossless / idk_id_instrument / idk_lossless, csrc/fqsx_idk.h) on the maxima over a file's id
    lines: False if the kernel would answer one of them with IDK_ERR_TOO_LONG.  Lossless mode: the line with its line feed within
    _ID_LINE_MAX bytes and within _ID_TOKENS_MAX tokens.  Instrument mode: the line within _ID_LINE_MAX; the name -- up to the
    first '.', ' ' or ':', cut short at a NUL -- within _ID_NAME_MAX bytes; and, as a new name is coded through the lossless path
    with a terminating NUL, the bytes up to the '.', ' ' or ':' within _ID_TOKENS_MAX tokens with that terminator.  (A line
    without a name, or with a byte >= 128 where it is coded, is refused by both coders: not a staging matter.)"""
    if max_line > _ID_LINE_MAX:
        return False
    if id_mode != "instrument":
        return max_tokens <= _ID_TOKENS_MAX
    return max_name <= _ID_NAME_MAX and max_name_tokens <= _ID_TOKENS_MAX


def _id_line_maxima(ids: np.ndarray, id_off: np.ndarray, names: bool = True):
    """(longest line, most tokens in a line, longest instrument name, most tokens up to a name's end plus its terminator) of the
    id lines `ids` (each with its line feed), in one pass: what _id_maxima_fit takes, and what DeviceColumns.id_survey() reports
    of a resident id column.  The last two are over the lines that have a name; names False: 0 for both, not looked for."""
    off = np.asarray(id_off).astype(np.int64)
    if len(off) < 2:
        return 0, 0, 0, 0
    start, stop = off[:-1], off[1:]
    ids = np.asarray(ids)
    seps = np.zeros(len(ids) + 1, dtype=np.int64)
    np.cumsum(~_ID_LITERAL[ids], out=seps[1:])
    line, tokens = int((stop - start).max()), int((seps[stop] - seps[start]).max())
    if not names:
        return line, tokens, 0, 0
    end = _first_at_or_after(np.flatnonzero(_ID_NAME_END[ids]), start, stop)
    named = end < stop
    if not bool(named.any()):
        return line, tokens, 0, 0
    name_len = _first_at_or_after(np.flatnonzero(ids == 0), start, end) - start
    return line, tokens, int(name_len[named].max()), int((seps[end] - seps[start] + 1)[named].max())


def _id_lines_fit_the_kernel(ids: np.ndarray, id_off: np.ndarray, id_mode: str) -> bool:
    """_id_maxima_fit for the id lines `ids` (each with its line feed)"""
    return _id_maxima_fit(id_mode, *_id_line_maxima(ids, id_off, names=id_mode == "instrument"))


def _ids_fit_the_kernel(id_mode: str, *recs) -> bool:
    """False if an id of the file is beyond what the GPU id coder stages (the host coder, like the reference, has no limits):
    a cheap pre-scan so that the file goes to the host coder as a whole instead of changing over in mid-file.  (What no
    pre-scan of lines can know, the number of different instrument names a worker meets, is left to that change-over.)"""
    return all(_id_lines_fit_the_kernel(*hp.id_arrays(rec, np.arange(len(rec))), id_mode) for rec in recs)


def _compress(inputs, ids_fit, threads: int, order: str, genome_size_mbp: int, quality_mode: str, id_mode: str, quality_thr: int, device: int,
              lib_path: Optional[str], as_blocks: bool, gpu_ids: Optional[bool], stats: Optional[dict], resident: bool = False,
              profile: bool = False, resident_ids: bool = False):
    """The file of one input (`fqs e -s`) or of two mate inputs (`fqs e -p`), each a hostpipe.Records, a hostpipe.Columns or
    -- resident -- a codec.DeviceColumns, which all cut a block's columns under the same names: block, ids_of, quals_of, with a
    mate block_pe, ids_of_pe, quals_of_pe (DeviceColumns: block_dev / block_pe_dev, the block cut on the device with its
    qualities; resident_ids: ids_dev / ids_pe_dev too, the id lines cut on the device for the id kernel, and ids_of / ids_of_pe
    for the host coder).  ids_fit(): the caller's pre-scan of the id lines, asked if gpu_ids is None.  Returns the file's bytes or
    -- as_blocks -- (header, generator of container blocks); resident columns are released behind the last block."""
    paired, c1, mates = len(inputs) == 2, inputs[0], inputs[1:]
    if gpu_ids is None:
        gpu_ids = id_mode == "none" or ids_fit()
    if stats is not None:
        stats["gpu_ids"] = gpu_ids
    mode = ("pe_" if paired else "se_") + ("sorted" if order == "s" else "original")
    header = hp.make_header(threads, mode, genome_size_mbp, quality_mode, id_mode, quality_thr)
    groups = _gpu_groups(c1, device, lib_path, stats) if order == "s" else None   # mates follow mate 1's order, io.h:541-550
    if resident and profile:
        c1.set_profiling(True)
    sizes = [c.record_sizes() for c in inputs]

    def cutter(name: str, dev: str = ""):
        """mate 1's method `name` on one input, its _pe form with the mate on two"""
        name += ("_pe" if paired else "") + dev
        return lambda idx: getattr(c1, name)(*mates, idx)
    block, ids_of, quals_of = cutter("block", "_dev" if resident else ""), cutter("ids_of"), cutter("quals_of")
    ids_dev = cutter("ids", "_dev")

    def ids_for_the_coder(idx):
        if id_mode == "none":
            return None, None
        if not resident_ids:
            return ids_of(idx)
        if not gpu_ids:   # (the host coder: its job cuts and downloads the lines, encode_blocks)
            return None, None
        blk = ids_dev(idx)
        return blk, blk.off

    def arrays(idx):
        ids, id_off = ids_for_the_coder(idx)
        if resident:
            blk = block(idx)
            return blk, blk.off, ids, id_off, None
        bases, off = block(idx)
        return bases, off, ids, id_off, quals_of(idx)[0] if quality_mode != "none" else None

    def sizes_of(idx):
        if not paired:
            return sizes[0][idx]
        z = np.empty(2 * len(idx), dtype=np.int64)
        z[0::2], z[1::2] = sizes[0][idx], sizes[1][idx]
        return z

    blocks = hp.form_blocks_pe(c1, *mates, mode, groups=groups) if paired else hp.form_blocks(c1, mode, groups=groups)
    gen = encode_blocks(header, blocks, arrays, sizes_of, paired, device, lib_path, stats=stats, gpu_ids=gpu_ids, ids_of=ids_of)
    if resident:
        gen = _closing_columns(gen, inputs, stats, profile)
    return (header, gen) if as_blocks else hp.write_fqs(header, gen)


def compress_records(rec: hp.Records, threads: int, order: str = "s", genome_size_mbp: int = 3100, device: int = 0,
                     lib_path: Optional[str] = None, quality_mode: str = "none", id_mode: str = "none",
                     quality_thr: int = 20, as_blocks: bool = False, gpu_ids: Optional[bool] = None, stats: Optional[dict] = None):
    """`fqs e -s -om <order> -t <threads> -gs <g> -qm <..> -im <..>` on single-end records.  Returns the file's bytes, or
    -- as_blocks -- (header, generator of container blocks) for files too large to hold (hostpipe.fqs_chunks serialises them).
    gpu_ids: the id stream from the GPU kernel (True), from the host coder (False: one thread per worker, no limits on the id
    lines), or -- None -- the kernel unless an id of the file is beyond its staging limits.  A file on the kernel that meets
    more instrument names than a worker's list holds goes on with the host coder from that block (the same bytes).  stats:
    "gpu_ids" (the choice made), "id_host_fallback" (changed over in mid-file) and what encode_blocks adds."""
    return _compress([rec], lambda: _ids_fit_the_kernel(id_mode, rec), threads, order, genome_size_mbp, quality_mode, id_mode, quality_thr,
                     device, lib_path, as_blocks, gpu_ids, stats)


def compress_records_pe(rec1: hp.Records, rec2: hp.Records, threads: int, order: str = "s", genome_size_mbp: int = 3100,
                        device: int = 0, lib_path: Optional[str] = None, quality_mode: str = "none", id_mode: str = "none",
                        quality_thr: int = 20, as_blocks: bool = False, gpu_ids: Optional[bool] = None, stats: Optional[dict] = None):
    """`fqs e -p ...` on two mate files (records interleaved mate 1 / mate 2 inside a block).  gpu_ids: see compress_records."""
    return _compress([rec1, rec2], lambda: _ids_fit_the_kernel(id_mode, rec1, rec2), threads, order, genome_size_mbp, quality_mode, id_mode,
                     quality_thr, device, lib_path, as_blocks, gpu_ids, stats)


def _id_columns_fit_the_kernel(cols: hp.Columns, max_id_line: int, id_mode: str) -> bool:
    """_ids_fit_the_kernel on columns: the parser's longest id line (it counts the line feed) and one pass over the id bytes."""
    return max_id_line <= _ID_LINE_MAX and _id_lines_fit_the_kernel(cols.ids, cols.id_off.view(np.int64), id_mode)


def compress_fastq(text_or_path, text2_or_path2=None, threads: int = 1, order: str = "s", genome_size_mbp: int = 3100,
                   quality_mode: str = "illumina_8", id_mode: str = "instrument", quality_thr: int = 20, device: int = 0,
                   lib_path: Optional[str] = None, as_blocks: bool = False, gpu_ids: Optional[bool] = None, stats: Optional[dict] = None,
                   max_chunk_bytes: int = 0, resident: bool = False, profile: bool = False, resident_ids: bool = False, inflate: str = "auto"):
    """`fqs e` on FASTQ files: `-s` with one input, `-p` with two (text as bytes / uint8 array, or a path; the defaults are the
    reference's, params.h:53-78; either input may be gzip, each on its own: BGZF is inflated on the GPU, other gzip by zlib on the
    host -- inflate, as codec.parse_fastq takes it, and stats["parse"][k]["inflate"]).  The text is parsed on the GPU into columns (codec.parse_fastq), the sort pre-pass runs on the
    base column, and the blocks are cut from the columns with vectorised gathers.  Returns what compress_records* return.
    ValueError: a record whose quality line differs in length from its base line; mate files with different numbers of records.
    gpu_ids: see compress_records.  stats: "parse" (one dict per input), "sort" (sorted order: what _gpu_groups reports of the
    pre-pass), "gpu_ids" (the choice made), "id_host_fallback" (the id coder changed over to the host coder in mid-file) and what
    encode_blocks adds.
    resident: the base and quality columns stay in device memory (codec.DeviceColumns, one store per input) and the blocks are
    cut there; the same bytes.  Neither column comes to the host: sorted order sorts mate 1's store where it lies
    (DeviceColumns.sort_order).  stats then also has "columns" (DeviceColumns.info() per input once the last block is written, with
    -- profile -- the gather kernel's "kernels").
    resident_ids (with resident; ValueError without): the id column stays in device memory too.  The pre-scan is the stores' id
    survey, a block's id lines are cut on the device and the id kernel reads them there; no id byte of the input comes to the host
    unless the host id coder is needed, which then downloads the blocks it codes.  The same bytes.  stats["ids_resident"]
    says so, and "columns" has the "id_bytes" held."""
    if resident_ids and not resident:
        raise ValueError("resident_ids needs resident: the id column stays beside the two others")
    paired = text2_or_path2 is not None
    cols, parse_stats = [], []
    try:
        for src in (text_or_path, text2_or_path2)[:2 if paired else 1]:
            st = {}
            try:
                cols.append(parse_fastq(src, device=device, lib_path=lib_path, max_chunk_bytes=max_chunk_bytes, stats=st, resident=resident,
                                        resident_ids=resident_ids, inflate=inflate))
            except LengthMismatch:   # (resident columns cannot hold such a record: parse_fastq stops at its chunk)
                st["length_mismatch"] = True
            parse_stats.append(st)
            if st["length_mismatch"]:
                raise ValueError("a record's quality line differs in length from its base line (input %d)" % len(parse_stats))
        if paired and len(cols[0]) != len(cols[1]):
            raise ValueError("the mate files hold different numbers of records: %d and %d" % (len(cols[0]), len(cols[1])))
        if stats is not None:
            stats["parse"] = parse_stats
            stats["ids_resident"] = resident_ids

        def ids_fit():
            if resident_ids:   # (the survey kernel on every store: the maxima alone come to the host)
                return all(_id_maxima_fit(id_mode, sv["max_line"], sv["max_tokens"], sv["max_name"], sv["max_name_tokens"])
                           for sv in (c.id_survey() for c in cols))
            return all(_id_columns_fit_the_kernel(c, st["max_id_line"], id_mode) for c, st in zip(cols, parse_stats))
        return _compress(cols, ids_fit, threads, order, genome_size_mbp, quality_mode, id_mode, quality_thr, device, lib_path, as_blocks, gpu_ids,
                         stats, resident, profile, resident_ids)
    except BaseException:
        if resident:
            for c in cols:
                c.close()
        raise


def _closing_columns(gen, cols, stats: Optional[dict], profile: bool):
    """the blocks of gen; then the device columns are released"""
    try:
        yield from gen
        if stats is not None:
            stats["columns"] = [dict(c.info(), **({"kernels": c.kernel_times()} if profile else {})) for c in cols]
    finally:
        for c in cols:
            c.close()


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
    ap.add_argument("-resident-ids", dest="resident_ids", action="store_true",
                    help="keep the id column in device memory too and cut the id lines there (implies -resident)")
    ap.add_argument("-inflate", choices=["auto", "device", "host"], default="auto",
                    help="gzip input: BGZF members on the GPU (device), zlib on the host (host), or the faster of the two for the file's kind (auto)")
    ap.add_argument("inputs", nargs="+")
    a = ap.parse_args(argv)
    if len(a.inputs) != (2 if a.paired else 1):
        ap.error("-p takes two input files, -s one")
    header, blocks = compress_fastq(a.inputs[0], a.inputs[1] if a.paired else None, threads=min(max(a.t, 1), 64), order=a.om,
                                    genome_size_mbp=min(max(a.gs, 1), 32768), quality_mode=_QM[a.qm], id_mode=_IM[a.im], quality_thr=a.qt,
                                    device=a.device, lib_path=a.lib, as_blocks=True, resident=a.resident or a.resident_ids,
                                    resident_ids=a.resident_ids, inflate=a.inflate)
    with open(a.out, "wb") as f:
        for chunk in hp.fqs_chunks(header, blocks):   # block by block: the file is never held whole
            f.write(chunk)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
