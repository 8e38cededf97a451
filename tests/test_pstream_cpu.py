"""The temporal post-hoc model file on the host: the container's round trip and bit budget, every refusal of read(), the
choice rule and the host oracle on constructed clips, the all-intra bound, and the tensor sections byte for byte as qstream / zstream write
them.  No GPU: the host coder of the library is host code."""
import io
import struct
from types import SimpleNamespace

import numpy as np
import pytest

import pstream_cases as PC

CLIPS = [("walk", PC.walk_clip), ("uniform", PC.uniform_clip), ("black", lambda n: PC.black_clip(n, n // 2))]


def _budget_ok(blob):
    from boosting_nerv_amd import pstream
    b = pstream.info(blob)
    assert b["total"] == 8 * len(blob) == 8 * b["bytes"] == sum(b[k] for k in pstream.ITEMS)
    return b


# ---------------------------------------------------------------------------------------------------------------------- container
@pytest.mark.parametrize("sparse", [False, True])
def test_round_trip_and_budget(sparse, tmp_path):
    from boosting_nerv_amd import codec, pstream
    q = PC.walk_clip(8)
    blob, settings, e = PC.file_of(q, sparse)
    path = tmp_path / "t.bnrp"
    _, lengths, records, words, _ = PC.tensor_section(sparse)
    assert pstream.write(str(path), settings, lengths, records, words, e) == len(blob) and path.read_bytes() == blob
    assert pstream.magic_of(blob) == pstream.MAGIC == b"BNRP"
    for src in (blob, io.BytesIO(blob), str(path)):
        ps = pstream.read(src)
        assert ps.settings == settings and np.array_equal(ps.lengths, lengths) and np.array_equal(ps.words, words) and len(ps.records) == len(records)
        for a, b in zip(ps.records, records):
            assert a[:5] == tuple(int(v) for v in b[:5]) and all(np.array_equal(x, y) for x, y in zip(a[-3:], b[-3:]))
        g = ps.embeds
        assert g.shape == e.shape and (g.outer, g.red, g.inner, g.dtype) == (e.outer, e.red, e.inner, e.dtype)
        for name in ("min", "scale", "lengths0", "lengths1", "pred", "run_bits", "words0", "words1"):
            assert np.array_equal(getattr(g, name), getattr(e, name)), name
        assert g.min.dtype == np.float32 and g.run_bits.shape == (8, 3)
    b = _budget_ok(blob)
    n_runs = 8 * 3
    assert b["embed_run_index"] == 16 * n_runs == 16 * b["n_embed_runs"] and b["embed_tables"] == 8 * 2 * 257
    assert b["embed_side"] == 8 * (16 + 16 + 4 + 4 + 8 + 4 + 4)        # shape, grid geometry, one fp32 pair, pred bytes, two word counts
    assert b["embed_symbol_bits"] == int(e.run_bits.sum()) == b["intra_frame_bits"] + b["inter_frame_bits"]
    assert b["n_embed_symbols"] == q.size and b["n_inter_frames"] + b["n_intra_frames"] == 8 and b["tensor_kind"] == ("sparse" if sparse else "dense")
    assert ("zero_parse" in b) == sparse and codec.info(blob) == b
    line = codec.describe_any(b)
    assert f"{len(blob)} bytes = {8 * len(blob)} bits" in line and f"{b['n_inter_frames']} as differences" in line and ("parse " in line) == sparse


@pytest.mark.parametrize("sparse", [False, True])
def test_tensor_section_is_byte_for_byte_the_section_of_the_plain_file(sparse):
    """The bytes between the header and the embedding section are those qstream / zstream write behind THEIR header for the same records."""
    from boosting_nerv_amd import pstream, qstream
    blob, settings, e = PC.file_of(PC.walk_clip(8), sparse)
    plain_settings, lengths, records, words, fmt = PC.tensor_section(sparse)
    plain = fmt.to_bytes(plain_settings, lengths, records, words)
    assert fmt.read(plain).settings == plain_settings
    head = lambda s: 20 + len(b"".join(qstream._header(s)))      # noqa: E731  (prefix, header length, header)
    section = plain[head(plain_settings):-4]
    assert len(section) > 1000 and blob[head(settings):head(settings) + len(section)] == section
    tail = b"".join(pstream._embed_section(e))
    assert blob[head(settings) + len(section):-4] == tail      # and nothing else lies between them


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_read_refuses_what_qstream_refuses():
    from boosting_nerv_amd import pstream
    q = PC.walk_clip(8)
    blob, settings, e = PC.file_of(q)
    for bad, what in ((blob[:10], "pstream: truncated"), (b"BNRQ" + blob[4:], "pstream: bad magic"), (blob[:4] + struct.pack("<I", 2) + blob[8:], "pstream: unknown format version"),
                      (blob[:-5] + blob[-4:], "pstream: truncated or padded"), (blob + b"\0", "pstream: truncated or padded"),
                      (blob[:100] + bytes([blob[100] ^ 1]) + blob[101:], "pstream: CRC mismatch")):
        with pytest.raises(ValueError, match=what):
            pstream.read(bad)
    payload = blob[16:-4]
    with pytest.raises(ValueError, match="pstream: the settings header is not JSON"):
        pstream.read(PC.frame(struct.pack("<I", 5) + b"{nope" + payload[4:]))
    with pytest.raises(ValueError, match="pstream: the settings header is not a JSON object"):
        pstream.read(PC.frame(struct.pack("<I", 2) + b"[]" + payload[4:]))
    with pytest.raises(ValueError, match="pstream: truncated"):          # a payload that ends inside the embedding section
        pstream.read(PC.frame(payload[:-7]))
    with pytest.raises(ValueError, match="pstream: 3 payload bytes follow"):
        pstream.read(PC.frame(payload + b"\0\0\0"))
    for run in (0, 2048, "256", None):
        with pytest.raises(ValueError, match="pstream: the header's run length"):
            pstream.read(PC.damaged(q, dict(settings, huff_run=run)))
    # the tensor section's own refusals, under this format's name
    _, lengths, records, words, fmt = PC.tensor_section()
    from boosting_nerv_amd import qstream

    def with_section(lengths=lengths, records=records, words=words):
        return PC.frame(b"".join(qstream._header(settings) + qstream._section(lengths, records, words) + pstream._embed_section(e)))

    assert pstream.read(with_section()).settings == settings
    long = lengths.copy()
    long[np.flatnonzero(lengths)[0]] = 33
    with pytest.raises(ValueError, match="pstream: a code length of 33 exceeds 32"):
        pstream.read(with_section(lengths=long))
    off = lengths.copy()
    off[np.flatnonzero(lengths)[0]] += 1
    with pytest.raises(ValueError, match="pstream: the code lengths break Kraft"):
        pstream.read(with_section(lengths=off))
    with pytest.raises(ValueError, match="pstream: a record of 700 elements with the grid"):
        pstream.read(with_section(records=[records[0]._replace(red=699)] + records[1:]))
    short = records[0]._replace(run_bits=records[0].run_bits - np.array([1, 0, 0], dtype=np.uint16))
    with pytest.raises(ValueError, match="pstream: the run lengths of the records add up"):
        pstream.read(with_section(records=[short] + records[1:], words=words[:-2]))


def test_read_refuses_a_damaged_embedding_section():
    from boosting_nerv_amd import pstream
    q = PC.walk_clip(8)
    blob, settings, e = PC.file_of(q)
    assert e.pred.tolist() == [0] + [1] * 7
    assert pstream.read(PC.damaged(q)).embeds.pred.tolist() == e.pred.tolist()       # the builder itself writes a good file
    for key in ("embed_pred", "tensor_kind"):
        with pytest.raises(ValueError, match=f"pstream: the header's {key}"):
            pstream.read(PC.damaged(q, {k: v for k, v in settings.items() if k != key}))
    with pytest.raises(ValueError, match="pstream: the header's embed_pred is 'next'"):
        pstream.read(PC.damaged(q, dict(settings, embed_pred="next")))
    pred = e.pred.copy()
    pred[3] = 2
    with pytest.raises(ValueError, match="pstream: a pred byte of 2"):
        pstream.read(PC.damaged(q, pred=pred))
    pred = e.pred.copy()
    pred[0] = 1
    with pytest.raises(ValueError, match=r"pstream: frame 0 is coded as a difference \(pred\[0\] = 1\)"):
        pstream.read(PC.damaged(q, pred=pred))
    with pytest.raises(ValueError, match="pstream: 7 frames are coded as differences, the inter code table is absent"):
        pstream.read(PC.damaged(q, lengths1=np.zeros(257, dtype=np.uint8)))
    with pytest.raises(ValueError, match="pstream: 8 frames of 576 elements with the grid"):
        pstream.read(PC.damaged(q, red=e.red - 1))
    with pytest.raises(ValueError, match="pstream: 8 frames of 576 elements with the grid"):
        pstream.read(PC.frame(_with_dtype_flag(blob, e, 2)))
    for t, name in ((0, "intra"), (5, "inter")):             # one run length altered by one: the sum leaves its string's word count ...
        rb = e.run_bits.copy()
        rb[t, 1] += 40
        with pytest.raises(ValueError, match=f"pstream: the run lengths of the {name} frames add up"):
            pstream.read(PC.damaged(q, run_bits=rb))
    moved = e.pred.copy()                                    # ... and a frame moved to the other string does too
    moved[4] = 0
    with pytest.raises(ValueError, match="pstream: the run lengths of the"):
        pstream.read(PC.damaged(q, pred=moved))
    bad = e.lengths1.copy()
    bad[np.flatnonzero(bad)[0]] += 1
    with pytest.raises(ValueError, match="pstream: the code lengths break Kraft"):
        pstream.read(PC.damaged(q, lengths1=bad))
    with pytest.raises(ValueError, match="pstream: the code lengths break Kraft"):      # the intra table is never absent: frame 0 needs it
        pstream.read(PC.damaged(q, lengths0=np.zeros(257, dtype=np.uint8)))


def _with_dtype_flag(blob, e, flag):
    """The payload of `blob` with the embedding grid's dtype flag overwritten."""
    from boosting_nerv_amd import pstream
    payload = bytearray(blob[16:-4])
    at = len(payload) - len(b"".join(pstream._embed_section(e))) + 16 + 12
    assert struct.unpack_from("<I", payload, at)[0] == e.dtype
    struct.pack_into("<I", payload, at, flag)
    return bytes(payload)


def test_writer_refuses_settings_without_the_two_keys():
    from boosting_nerv_amd import pstream
    _, settings, e = PC.file_of(PC.walk_clip(2))
    _, lengths, records, words, _ = PC.tensor_section()
    for key in ("embed_pred", "tensor_kind"):
        with pytest.raises(ValueError, match="pstream.write"):
            pstream.to_bytes({k: v for k, v in settings.items() if k != key}, lengths, records, words, e)


# ---------------------------------------------------------------------------------------------------------------------- the choice rule
def _section_of(q):
    from boosting_nerv_amd import codec, pstream
    lengths0, lengths1, pred, run_bits, words0, words1 = codec.code_embeds(q)
    written = pstream.section_bits(q.shape[0], q.shape[1], words0.size, words1.size)
    return pred, lengths0, lengths1, run_bits, written


@pytest.mark.parametrize("n", [8, 70])
@pytest.mark.parametrize("name,make", CLIPS)
def test_choice_oracle_and_bound_on_constructed_clips(name, make, n):
    from boosting_nerv_amd import pstream
    q = make(n)
    assert q.shape == (n, PC.P)
    pred, lengths0, lengths1, run_bits, written = _section_of(q)
    d, h0, h1 = pstream.symbols(q)
    want = pstream.choose(h0, h1)
    assert np.array_equal(want[0], pred) and np.array_equal(want[1], lengths0) and np.array_equal(want[2], lengths1)
    assert written <= pstream.all_intra_section_bits(q)       # the bound
    if name == "walk":
        assert pred.tolist() == [0] + [1] * (n - 1) and lengths1.any()
        assert written < pstream.all_intra_section_bits(q) // 2
    elif name == "uniform":
        assert not pred.any() and not lengths1.any() and written == pstream.all_intra_section_bits(q)
    else:
        cut = n // 2
        assert pred[cut] == 0 and pred[0] == 0 and pred[1:cut].all() and pred[cut + 2:].all()
        assert lengths0[0] != 0                              # the black frame's one symbol has a code in the intra table
    blob, _, e = PC.file_of(q)
    ps = pstream.read(blob)
    assert np.array_equal(ps.embeds.pred, pred) and np.array_equal(ps.embeds.run_bits, run_bits)
    assert np.array_equal(pstream.decode_embeds(ps), q)       # the wrap 255 -> 0 included: the chain is exact mod 256
    b = _budget_ok(blob)
    assert b["embed_section_bits"] == written and b["n_inter_frames"] == int(pred.sum())
    sym = np.where(pred[:, None] != 0, d, q)
    assert np.array_equal(PC.chain(sym, pred), q)


def test_one_frame():
    from boosting_nerv_amd import pstream
    q = PC.walk_clip(1)
    pred, lengths0, lengths1, run_bits, written = _section_of(q)
    assert pred.tolist() == [0] and not lengths1.any() and run_bits.shape == (1, 3) and written == pstream.all_intra_section_bits(q)
    blob, _, _ = PC.file_of(q)
    ps = pstream.read(blob)
    assert ps.embeds.words1.size == 0 and np.array_equal(pstream.decode_embeds(ps), q)
    b = _budget_ok(blob)
    assert b["n_inter_frames"] == 0 and b["n_intra_frames"] == 1 and b["inter_frame_bits"] == 0


def test_step_four_falls_back_when_two_strings_need_more_words_than_one():
    from boosting_nerv_amd import codec, pstream
    q = PC.tiny_fallback_clip()
    d, h0, h1 = pstream.symbols(q)
    all0, trial1 = codec.huffman_lengths(h0.sum(0)), codec.huffman_lengths(h1[1:].sum(0))
    assert int((h1[1] * trial1[:256]).sum()) == 8 < int((h0[1] * all0[:256]).sum()) == 12      # step 2 alone would make frame 1 inter
    pred, lengths0, lengths1 = pstream.choose(h0, h1)
    assert not pred.any() and not lengths1.any() and np.array_equal(lengths0, all0)
    lengths0, lengths1, pred, run_bits, words0, words1 = codec.code_embeds(q)
    assert words0.size == 1 and words1.size == 0 and run_bits.tolist() == [[12], [12]]


def test_choose_ties_go_to_intra_and_histograms_are_checked():
    from boosting_nerv_amd import pstream
    h0 = np.zeros((3, 256), dtype=np.int64)
    h0[:, 5] = 300
    h0[:, 9] = 276
    h1 = h0.copy()                                           # every frame costs the same either way
    pred, _, lengths1 = pstream.choose(h0, h1)
    assert not pred.any() and not lengths1.any()
    with pytest.raises(ValueError, match="pstream.choose"):
        pstream.choose(h0, h1[:2])
    with pytest.raises(ValueError, match="pstream: the codes of the embeddings"):
        pstream.symbols(np.zeros((0, 4), dtype=np.uint8))


def test_symbols_are_differences_mod_256_with_their_histograms():
    from boosting_nerv_amd import pstream
    q = np.array([[0, 255, 10, 200], [255, 0, 10, 100], [1, 1, 1, 1]], dtype=np.uint8)
    d, h0, h1 = pstream.symbols(q)
    assert d.tolist() == [[0, 0, 0, 0], [255, 1, 0, 156], [2, 1, 247, 157]]
    assert h0[2, 1] == 4 and h0.sum(1).tolist() == [4, 4, 4] and h1.sum(1).tolist() == [0, 4, 4] and h1[1, 156] == 1


# ---------------------------------------------------------------------------------------------------------------------- flags
def test_flag_checks_raise_value_error_before_anything_runs():
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    with pytest.raises(ValueError, match="--bitstream_temporal: the temporal kind is what --bitstream FILE writes"):
        codec.check_posthoc_flags(SimpleNamespace(model="HNeRV", bitstream=None, bitstream_temporal=True))
    with pytest.raises(ValueError, match="--bitstream_temporal: --model NeRV_Boost has no frame embeddings"):
        codec.check_posthoc_flags(SimpleNamespace(model="NeRV_Boost", bitstream="t.bnrp", bitstream_temporal=True))
    codec.check_posthoc_flags(SimpleNamespace(model="HNeRV_Boost", bitstream="t.bnrp", bitstream_temporal=True))
    codec.check_posthoc_flags(SimpleNamespace(model="NeRV_Boost", bitstream="t.bnrq"))
    args = T.build_parser().parse_args([])
    assert args.bitstream_temporal is False                  # off by default
    assert T.build_parser().parse_args(["--bitstream_temporal"]).bitstream_temporal is True


def test_repack_keeps_refusing_post_hoc_files():
    from boosting_nerv_amd import codec
    blob, _, _ = PC.file_of(PC.walk_clip(2))
    with pytest.raises(NotImplementedError, match="a post-hoc file is not repacked"):
        codec.repack(blob, io.BytesIO())
