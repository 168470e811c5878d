"""Every device allocation of the side-stream codecs may fail, and the call that met the failure can be repeated: with
FQSX_TEST_ALLOC_FAIL=k the k-th allocation of a codec's context is refused (fqsx_rt.h: dalloc).  For k = 0, 1, 2, ... a fresh
codec runs three blocks, small -> large -> small (the second outgrows every per-block buffer and both kinds of table);
a creation that fails must fail with FQSX_E_NOMEM, a block call that fails must do so too and is then repeated, without the
variable, on the same codec.  Every block's output and the final per-worker state must equal those of the run nothing was
injected into: a buffer that was handed back is forgotten before its successor is asked for (dfit), a table stays in place
until its successor is filled (hash_tab_regrow), and nothing is launched before the block has all its memory.

Block calls that failed per case before the sweep ended at the first k nothing failed for (the emulation build; the device
build makes the same allocations): quality encode 9 (k = 3..11), quality decode 7 (3..9), id encode 12 (5..16), id decode 18
(5..22: with FQSX_IDG_INIT=16 the decoder doubles its output and its tables from 16 slots, a snapshot buffer with every table)."""
import re

import numpy as np
import pytest

from conftest import EMU_LIB
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.synth import synth_ids_varied, synth_quals

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
VAR = "FQSX_TEST_ALLOC_FAIL"
NOMEM = -4   # FQSX_E_NOMEM, include/fqsx.h
T = 3


def _code(err) -> int:
    """the library's return code out of an FqsxError ('<function>: <code>: <message>')"""
    m = re.match(r"\w+: (-?\d+): ", str(err))
    assert m, f"no return code in {err!r}"
    return int(m.group(1))


def _qual_blocks():
    """64 reads x 50 (fixed length), 301 pairs of ragged mates (reads of about 200 symbols: 602 reads, so that the inner
    boundaries of the three workers, 200.67 and 401.33, are rounded down to even), 64 x 50"""
    def fixed(n, L, seed):
        return synth_quals(n, L, seed).reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    rng = np.random.default_rng(77)
    lens = np.empty(602, dtype=np.int64)
    lens[0::2], lens[1::2] = rng.integers(180, 230, 301), rng.integers(150, 215, 301)
    off = np.zeros(603, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return [fixed(64, 50, 1), (synth_quals(1, int(off[-1]), 2).reshape(-1), off), fixed(64, 50, 3)]


def _id_blocks():
    """100 lines, 1000 pairs (mate suffixes), 100 lines; the lines of a block with their line feeds and offsets"""
    def arrays(lines):
        off = np.zeros(len(lines) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) + 1 for x in lines])
        return np.frombuffer(b"".join(x + b"\n" for x in lines), dtype=np.uint8), off
    m1, m2 = synth_ids_varied(1000, 12, mate=1), synth_ids_varied(1000, 12, mate=2)
    pairs = [x for ab in zip(m1, m2) for x in ab]
    return [arrays(synth_ids_varied(100, 11)) + (False,), arrays(pairs) + (True,), arrays(synth_ids_varied(100, 13)) + (False,)]


def _case(name, where):
    """(make a codec, [one call per block: codec -> comparable output], codec -> final state)"""
    from fqsqueezer_amd.codec import IdCodec, QualCodec
    kw = {"lib_path": EMU_LIB} if where == "emu" else {}
    if name.startswith("qual"):
        header = hp.make_header(T, "pe_original", 1, "lossless")
        make = lambda: QualCodec(header, device=0, **kw)   # noqa: E731
        blocks = _qual_blocks()
        state = lambda c: c.contexts()["per_worker"]   # noqa: E731
        if name == "qual_encode":
            return make, [lambda c, b=b: c.encode_block(*b) for b in blocks], state
        enc = make()
        streams = [enc.encode_block(*b) for b in blocks]
        return make, [lambda c, s=s, b=b: c.decode_block(s, b[1]).tobytes() for s, b in zip(streams, blocks)], state
    # (the decode case in instrument mode: the decoder's snapshot of the move-to-front names is one of its allocations)
    header = hp.make_header(T, "pe_original", 1, id_mode="instrument" if name == "id_decode" else "lossless")
    make = lambda: IdCodec(header, device=0, **kw)   # noqa: E731
    blocks = _id_blocks()
    state = lambda c: c.state().tolist()   # noqa: E731
    if name == "id_encode":
        return make, [lambda c, b=b: c.encode_block(*b) for b in blocks], state
    enc = make()
    streams = [enc.encode_block(*b) for b in blocks]

    def dec(c, s, b):
        ids, off = c.decode_block(s, len(b[1]) - 1, b[2])
        return ids.tobytes(), off.tolist()
    return make, [lambda c, s=s, b=b: dec(c, s, b) for s, b in zip(streams, blocks)], state


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", ["qual_encode", "qual_decode", "id_encode", "id_decode"])
def test_every_allocation_may_fail_and_the_call_be_repeated(where, request, monkeypatch, name):
    from fqsqueezer_amd.codec import FqsxError
    if where == "emu":
        request.getfixturevalue("built")
    monkeypatch.delenv(VAR, raising=False)
    monkeypatch.setenv("FQSX_IDG_INIT", "16")   # (read when a codec is created: both id model tables grow from 16 slots)
    make, calls, state = _case(name, where)
    ref = make()
    want = [call(ref) for call in calls]
    want_state = state(ref)
    failed_in_block = []
    for k in range(64):
        monkeypatch.setenv(VAR, str(k))
        try:
            codec = make()
        except FqsxError as e:
            assert _code(e) == NOMEM and VAR in str(e), f"k = {k}: creation failed with {e}"
            continue
        n_failed = 0
        for b, call in enumerate(calls):
            monkeypatch.setenv(VAR, str(k))
            try:
                got = call(codec)
            except FqsxError as e:
                assert _code(e) == NOMEM and VAR in str(e), f"k = {k}, block {b}: {e}"
                n_failed += 1
                monkeypatch.delenv(VAR)
                got = call(codec)   # the same call again, on the same codec
            assert got == want[b], f"k = {k}: block {b} differs from the run without a failure"
        assert state(codec) == want_state, f"k = {k}: the codec's final state differs"
        assert n_failed <= 1
        if not n_failed:
            break
        failed_in_block.append(k)
    else:
        pytest.fail("an allocation still failed at k = 63")
    monkeypatch.delenv(VAR, raising=False)
    print(f"{name} [{where}]: block calls failed for k = {failed_in_block}")
    assert len(failed_in_block) >= 3, f"only k = {failed_in_block} failed inside a block call"
