"""Read a `.fqs` file back: the bases and qualities of its reads, decoded on the GPU (codec.DnaCodec.decode_block,
codec.QualCodec.decode_block) from the read lengths of the meta stream (codec.MetaCodec.decode_block, host).  Works on the
files fqsfile writes and on those of the reference's `fqs e`.  The read-id stream is not decoded yet: a file that carries
one is accepted and the stream is skipped; writing FASTQ text is left to the caller until ids can be restored."""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import numpy as np

from . import hostpipe as hp
from .codec import DnaCodec, MetaCodec, QualCodec


def decompress_reads(data: bytes, device: int = 0, lib_path: Optional[str] = None) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """Generator over the container blocks of a .fqs file, in file order: (read_len uint32[n], bases uint8, quals uint8), the
    reads of a block back to back (mates interleaved mate 1 / mate 2 in paired files).  Per block the meta stream gives the
    read offsets, then the DNA kernels and the quality kernel decode side by side on their own HIP streams, as
    fqsfile.encode_blocks runs the encoders.  quality_mode none: every quality is 33 + quality_thr (quality.cpp:177-183)."""
    from concurrent.futures import ThreadPoolExecutor
    header, blocks = hp.parse_fqs(data)
    threads, paired = header[4], header[5] >= 2
    stored = hp.stored_streams(header)
    dna = DnaCodec(header, device=device, lib_path=lib_path)
    meta = MetaCodec(threads, lib_path=lib_path)
    qual = QualCodec(header, device=device, lib_path=lib_path) if hp.STREAM_QUALITY in stored else None
    pool = ThreadPoolExecutor(max_workers=2)
    try:
        for g, blk in enumerate(blocks):
            st = lambda sid: [blk.streams[w][sid] for w in range(threads)]   # noqa: E731
            read_len = meta.decode_block(st(hp.STREAM_META), blk.n_reads, paired)
            off = np.zeros(blk.n_reads + 1, dtype=np.uint64)
            off[1:] = np.cumsum(read_len, dtype=np.uint64)
            jd = pool.submit(dna.decode_block, st(hp.STREAM_DNA), off, g)
            if qual is not None:
                quals = pool.submit(qual.decode_block, st(hp.STREAM_QUALITY), off).result()
            else:
                quals = np.full(int(off[-1]), 33 + header[8], dtype=np.uint8)
            yield read_len, jd.result(), quals
    finally:
        pool.shutdown(wait=True)
        dna.close()
        meta.close()
        if qual is not None:
            qual.close()
