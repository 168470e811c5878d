"""Read a `.fqs` file back: the bases and qualities of its reads, decoded on the GPU (codec.DnaCodec.decode_block,
codec.QualCodec.decode_block) from the read lengths of the meta stream (codec.MetaCodec.decode_block, host).  Works on the
files fqsfile writes and on those of the reference's `fqs e`.  decompress_reads gives lengths, bases and qualities (the id
stream, if the file has one, is skipped); decompress_records also restores the read ids (codec.IdCodec.decode_block: the GPU id
decoder on a stream of its own, the host decoder for files whose ids are beyond the kernel's staging limits) and
decompress_fastq assembles the FASTQ text `fqs d` writes.  decompress_fastq_chunks is the streaming form: the file is read block
by block (hostpipe.iter_fqs), the decoders leave their columns on the device, the text is assembled there
(codec.FastqText) and comes back one container block at a time.  Command line: python -m fqsqueezer_amd.fqsread d in.fqs
-out a.fq [-out2 b.fq] [-host-text], which writes every block's text as it arrives."""
from __future__ import annotations

import os
from contextlib import closing
from typing import Iterator, Optional, Tuple, Union

import numpy as np

from . import hostpipe as hp
from .codec import DnaCodec, FastqText, IdFallback, MetaCodec, QualCodec


def _qual_fill(header: bytes) -> int:
    """quality_mode none: every quality is 33 + quality_thr (quality.cpp:177-183)"""
    return 33 + header[8]


def _decode_blocks(header: bytes, blocks, device: int, lib_path: Optional[str], with_ids: bool, dev: bool, gpu_ids: bool = True,
                   stats: Optional[dict] = None):
    """The one per-block decode loop: a generator over the container blocks `blocks` (hostpipe.FqsBlock, in file order) of the
    file with this header, each item (read_len uint32[n], off uint64[n + 1], bases, quals, ids).  Per block the id decoder
    starts on its own HIP stream, the meta stream gives the read offsets on the calling thread, then the DNA kernels and the
    quality kernel decode side by side on their own HIP streams, as fqsfile.encode_blocks runs the encoders.
    dev False: bases and quals are uint8 arrays, the reads back to back (quality_mode none: the constant fill), and ids is
    (ids uint8[], id_off uint64[n + 1]) (id_mode none: every id line is '@', id.cpp:486-492).
    dev True: the columns stay in device memory for codec.FastqText.block -- bases and quals are device pointers (quals None:
    the assembler fills in _qual_fill) and ids is (d_ids, d_id_len, id_bytes), or the same as host arrays once the host id
    decoder has taken over (codec.IdFallback), or (None, None, None): the assembler's constant id line.  The pointers are the
    decoders' own buffers, valid until this generator is resumed.
    with_ids False: no id decoder is opened and ids is None.  stats: receives 'id_host_fallback' and the id decoder's growth
    counters when the generator ends or is closed."""
    from concurrent.futures import ThreadPoolExecutor
    threads, paired = header[4], header[5] >= 2
    stored = hp.stored_streams(header)

    def decode_ids(dec, block, _):
        if dev and idd.on_gpu:   # (what the assembler takes: device pointers from the id kernel, host arrays with their lengths from the host decoder)
            return dec.decode_block_dev(*block, paired)
        ids, id_off = dec.decode_block(*block, paired)
        return (ids, np.diff(id_off).astype(np.uint32), len(ids)) if dev else (ids, id_off)

    opened = []   # every codec opened so far: closed again also if a later constructor raises

    def opening(codec):
        opened.append(codec)
        return codec
    idd = None
    pool = ThreadPoolExecutor(max_workers=3)
    try:
        dna = opening(DnaCodec(header, device=device, lib_path=lib_path))
        meta = opening(MetaCodec(threads, lib_path=lib_path))
        qual = opening(QualCodec(header, device=device, lib_path=lib_path)) if hp.STREAM_QUALITY in stored else None
        if with_ids and hp.STREAM_ID in stored:
            idd = opening(IdFallback(header, device, lib_path, gpu_ids, decode_ids))
        for g, blk in enumerate(blocks):
            st = lambda sid: [blk.streams[w][sid] for w in range(threads)]   # noqa: E731
            n = blk.n_reads
            ji = pool.submit(idd.run, (st(hp.STREAM_ID), n)) if idd is not None else None
            read_len = meta.decode_block(st(hp.STREAM_META), n, paired)
            off = np.zeros(n + 1, dtype=np.uint64)
            off[1:] = np.cumsum(read_len, dtype=np.uint64)
            jd = pool.submit(dna.decode_block_dev if dev else dna.decode_block, st(hp.STREAM_DNA), off, g)
            if qual is not None:
                quals = pool.submit(qual.decode_block_dev if dev else qual.decode_block, st(hp.STREAM_QUALITY), off).result()
            else:
                quals = None if dev else np.full(int(off[-1]), _qual_fill(header), dtype=np.uint8)
            bases = jd.result()
            if ji is not None:
                ids = ji.result()
            elif not with_ids:
                ids = None
            elif dev:
                ids = (None, None, None)
            else:
                ids = (np.tile(np.frombuffer(b"@\n", dtype=np.uint8), n), np.arange(n + 1, dtype=np.uint64) * np.uint64(2))
            yield read_len, off, bases, quals, ids
    finally:
        pool.shutdown(wait=True)
        if stats is not None and idd is not None:   # (here, so that a caller that stops after the last block has them too)
            stats["id_host_fallback"] = idd.fell_back
            if idd.on_gpu:
                stats["id_decoder"] = idd.codec.stats()
        for c in opened:
            c.close()


def decompress_reads(data: bytes, device: int = 0, lib_path: Optional[str] = None) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """Generator over the container blocks of a .fqs file, in file order: (read_len uint32[n], bases uint8, quals uint8), the
    reads of a block back to back (mates interleaved mate 1 / mate 2 in paired files), decoded by _decode_blocks.
    quality_mode none: every quality is 33 + quality_thr (quality.cpp:177-183)."""
    header, blocks = hp.parse_fqs(data)
    with closing(_decode_blocks(header, blocks, device, lib_path, with_ids=False, dev=False)) as decoded:
        for read_len, _, bases, quals, _ in decoded:
            yield read_len, bases, quals


def decompress_records(data: bytes, device: int = 0, lib_path: Optional[str] = None, stats: Optional[dict] = None,
                       gpu_ids: bool = True) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
    """decompress_reads with the read ids: per container block (read_len, bases, quals, ids uint8[], id_off uint64[n + 1]), the
    id lines each with its line feed, as the reference's decoder writes them (numeric fields without leading zeros, instrument
    mode: the instrument name only).  The id decoder runs on its own HIP stream beside the DNA and the quality decoder.
    id_mode none: every id is '@' (id.cpp:486-492).  stats: receives 'id_host_fallback' and the id decoder's growth counters."""
    header, blocks = hp.parse_fqs(data)
    with closing(_decode_blocks(header, blocks, device, lib_path, with_ids=True, dev=False, gpu_ids=gpu_ids, stats=stats)) as decoded:
        for read_len, _, bases, quals, (ids, id_off) in decoded:
            yield read_len, bases, quals, ids, id_off


def _scatter(dst: np.ndarray, at: np.ndarray, src: np.ndarray, off: np.ndarray) -> None:
    """dst[at[i] : at[i] + len_i] = src[off[i] : off[i + 1]] for every i, without a loop over i"""
    off = off.astype(np.int64)
    n = int(off[-1] - off[0])
    if n:
        dst[np.repeat(at - off[:-1], np.diff(off)) + np.arange(off[0], off[0] + n, dtype=np.int64)] = src[off[0]:off[0] + n]


def _take(src: np.ndarray, off: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """the segments src[off[i] : off[i + 1]], i in idx, back to back"""
    ln = off[idx + 1] - off[idx]
    at = np.zeros(len(idx) + 1, dtype=np.int64)
    at[1:] = np.cumsum(ln)
    return src[np.repeat(off[idx] - at[:-1], ln) + np.arange(int(at[-1]), dtype=np.int64)]


def fastq_text(read_len: np.ndarray, bases: np.ndarray, quals: np.ndarray, ids: np.ndarray, id_off: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The FASTQ text of the reads of a block, in their order: per read id line + bases + "\n+\n" + qualities + "\n"
    (application.cpp:871-889).  Returns (text uint8[], rec_off int64[n + 1])."""
    L = read_len.astype(np.int64)
    il = np.diff(id_off.astype(np.int64))
    rec_off = np.zeros(len(L) + 1, dtype=np.int64)
    rec_off[1:] = np.cumsum(il + 2 * L + 4)
    out = np.empty(int(rec_off[-1]), dtype=np.uint8)
    roff = np.zeros(len(L) + 1, dtype=np.int64)
    roff[1:] = np.cumsum(L)
    start = rec_off[:-1]
    _scatter(out, start, ids, id_off)
    _scatter(out, start + il, bases, roff)
    sep = start + il + L
    out[sep], out[sep + 1], out[sep + 2] = 10, ord("+"), 10
    _scatter(out, sep + 3, quals, roff)
    out[rec_off[1:] - 1] = 10
    return out, rec_off


def decompress_fastq(data: bytes, device: int = 0, lib_path: Optional[str] = None, stats: Optional[dict] = None,
                     gpu_ids: bool = True) -> Union[bytes, Tuple[bytes, bytes]]:
    """The FASTQ text `fqs d` writes for the file: bytes for a single-end file, (mate 1 file, mate 2 file) for a paired one
    (workers in order, blocks in file order, mates alternately to the two outputs: application.cpp:871-889, 980-982)."""
    if len(data) < 18 or data[0] != 17:
        raise ValueError("not a .fqs file (header length byte)")
    paired = data[6] >= 2   # header byte 5: the DNA mode
    parts: Tuple[list, list] = ([], [])
    for read_len, bases, quals, ids, id_off in decompress_records(data, device=device, lib_path=lib_path, stats=stats, gpu_ids=gpu_ids):
        text, rec_off = fastq_text(read_len, bases, quals, ids, id_off)
        if not paired:
            parts[0].append(text.tobytes())
            continue
        for m in (0, 1):   # record i of the block goes to file i & 1
            parts[m].append(_take(text, rec_off, np.arange(m, len(read_len), 2, dtype=np.int64)).tobytes())
    return (b"".join(parts[0]), b"".join(parts[1])) if paired else b"".join(parts[0])


def _mates(text: np.ndarray, rec_off: np.ndarray, paired: bool):
    """a block's text as decompress_fastq_chunks yields it: record i of a paired block goes to output i & 1"""
    if not paired:
        return text.tobytes()
    n = len(rec_off) - 1
    return tuple(_take(text, rec_off, np.arange(m, n, 2, dtype=np.int64)).tobytes() for m in (0, 1))


def decompress_fastq_chunks(src, device: int = 0, lib_path: Optional[str] = None, stats: Optional[dict] = None, gpu_ids: bool = True,
                            gpu_text: bool = True) -> Iterator[Union[bytes, Tuple[bytes, bytes]]]:
    """decompress_fastq block by block: a generator over the container blocks of the file `src` (a path, a binary file object
    or bytes), each item the FASTQ text of one block -- bytes for a single-end file, (mate 1 text, mate 2 text) for a paired
    one.  The file is read as the blocks are asked for (hostpipe.iter_fqs).  Per block the meta stream is decoded on the host,
    the DNA, quality and id decoders run side by side and leave their columns in device memory, codec.FastqText assembles
    the text there, and its download runs on a worker thread while the next block decodes: a run holds one block of streams
    and two blocks of text.  quality_mode none: the assembler fills in 33 + quality_thr; id_mode none: its constant id line.
    After a staging-limit fallback of the id decoder (codec.IdFallback) the ids reach the assembler as host arrays.  gpu_text=False: the
    same chunks through the decoders' host entry points and fastq_text / _take.  stats: as decompress_records, plus 'text':
    {'gpu_text', 'bytes': [mate 1, mate 2], 'blocks'} and -- stats['profile_text'] set by the caller -- 'kernels'."""
    import io
    from concurrent.futures import ThreadPoolExecutor
    own = isinstance(src, (bytes, bytearray, memoryview, str, os.PathLike))
    f = io.BytesIO(src) if isinstance(src, (bytes, bytearray, memoryview)) else open(src, "rb") if own else src
    decoded = text = None
    loader = ThreadPoolExecutor(max_workers=1)   # downloads the text of the block assembled last
    written, n_blocks = [0, 0], 0
    try:
        blocks = hp.iter_fqs(f)
        header = next(blocks)
        paired = header[5] >= 2
        if gpu_text:
            text = FastqText(device=device, lib_path=lib_path)
            text.set_profiling(bool(stats and stats.get("profile_text")))
        decoded = _decode_blocks(header, blocks, device, lib_path, with_ids=True, dev=bool(gpu_text), gpu_ids=gpu_ids, stats=stats)

        def download():
            return (text.download(0).tobytes(), text.download(1).tobytes()) if paired else text.download(0).tobytes()

        def count(chunk):
            nonlocal n_blocks
            n_blocks += 1
            for m, part in enumerate(chunk if paired else (chunk,)):
                written[m] += len(part)
            return chunk

        pending = None   # the download of the block assembled last
        for read_len, off, bases, quals, ids in decoded:
            if not gpu_text:
                yield count(_mates(*fastq_text(read_len, bases, quals, *ids), paired))
                continue
            done = pending.result() if pending is not None else None   # (one call at a time on the assembler's handle)
            text.block(off, bases, quals, ids=ids[0], id_len=ids[1], id_bytes=ids[2], paired=paired, qual_fill=_qual_fill(header))
            pending = loader.submit(download)
            if done is not None:
                yield count(done)
        if pending is not None:
            done, pending = pending.result(), None
            yield count(done)
    finally:
        loader.shutdown(wait=True)
        if stats is not None:
            stats["text"] = {"gpu_text": bool(gpu_text), "bytes": list(written), "blocks": n_blocks}
            if text is not None and stats.get("profile_text"):
                stats["text"]["kernels"] = text.kernel_times()
        if decoded is not None:
            decoded.close()   # (fills in the id decoder's part of stats and closes the decoders)
        if text is not None:
            text.close()
        if own:
            f.close()


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m fqsqueezer_amd.fqsread", description="decompress a .fqs file to FASTQ on the GPU")
    ap.add_argument("cmd", choices=["d"])
    ap.add_argument("input")
    ap.add_argument("-out", required=True)
    ap.add_argument("-out2")
    ap.add_argument("-device", type=int, default=0)
    ap.add_argument("-lib", default=None, help="path of the library to load (default: the package's libfqsx.so)")
    ap.add_argument("-host-text", dest="host_text", action="store_true", help="assemble the FASTQ text on the host instead of the GPU")
    a = ap.parse_args(argv)
    with open(a.input, "rb") as f:
        head = f.read(18)
        if len(head) < 18 or head[0] != 17:
            raise ValueError("not a .fqs file (header length byte)")
        paired = head[6] >= 2   # header byte 5: the DNA mode
        if paired and not a.out2:
            ap.error("a paired file needs -out2")
        f.seek(0)
        with open(a.out, "wb") as o1, (open(a.out2, "wb") if paired else open(os.devnull, "wb")) as o2:
            for chunk in decompress_fastq_chunks(f, device=a.device, lib_path=a.lib, gpu_text=not a.host_text):
                if paired:
                    o1.write(chunk[0])
                    o2.write(chunk[1])
                else:
                    o1.write(chunk)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
