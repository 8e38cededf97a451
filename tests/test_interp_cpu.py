"""The interpolation file on the host: the rule that says which frames are stored and how every other frame's embedding
follows from theirs, its numpy restatement, the flag's parse-time refusals, and the header key through the three post-hoc containers.  No GPU."""
import json
import struct
import zlib

import numpy as np
import pytest
import torch

import pstream_cases as PC
from interp_cases import PLANS, rows


# ---------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("n,split", sorted(PLANS))
def test_interp_plan_cases(n, split):
    from boosting_nerv_amd.hnerv_utils import INTERP_ENTRY, data_split, interp_plan
    stored, plan = interp_plan(n, split)
    want_stored, want_rows = PLANS[(n, split)]
    assert stored == want_stored == data_split(list(range(n)), [int(x) for x in split.split("_")], False)[0]
    assert plan.dtype == INTERP_ENTRY and plan.shape == (n,) and plan.dtype.itemsize == 12 and plan["w"].dtype == np.float32
    assert rows(plan) == want_rows
    for k, t in enumerate(stored):                         # a stored frame is its own row
        assert rows(plan)[t] == (k, k, 0.0)


def test_interp_plan_weights_are_fp32_quotients():
    from boosting_nerv_amd.hnerv_utils import interp_plan
    _, plan = interp_plan(5, "1_1_3")
    assert plan["w"][1] == np.float32(1) / np.float32(3) and plan["w"][2] == np.float32(2) / np.float32(3)
    assert float(plan["w"][1]) != 1 / 3                    # (the fp32 quotient, not the double)
    _, plan = interp_plan(5, "1_1_2")
    assert plan["w"][1] == np.float32(0.5) and plan["w"][3] == np.float32(0.5)


def test_interp_plan_is_the_reference_rule_for_1_1_2():
    """--interpolation keeps an odd frame count: every held-out frame idx has the stored neighbours idx - 1 and idx + 1 at w = 0.5."""
    from boosting_nerv_amd.hnerv_utils import interp_plan
    for n in (3, 7, 17):
        stored, plan = interp_plan(n, "1_1_2")
        assert stored == list(range(0, n, 2))
        for t in range(1, n, 2):
            ia, ib, w = rows(plan)[t]
            assert (stored[ia], stored[ib], w) == (t - 1, t + 1, 0.5)


def test_interp_plan_refusals():
    from boosting_nerv_amd.hnerv_utils import check_interp_plan, interp_plan
    with pytest.raises(ValueError, match="stores no frame"):
        interp_plan(5, "0_1_2")
    with pytest.raises(ValueError, match="stores no frame"):
        interp_plan(0, "1_1_2")
    with pytest.raises(ValueError, match="--shuffle_data"):
        interp_plan(5, "1_1_2", shuffle_data=True)
    _, plan = interp_plan(5, "1_1_2")
    assert check_interp_plan(plan, 3) is not None
    with pytest.raises(ValueError, match="outside 0..1"):
        check_interp_plan(plan, 2)
    for bad in (1.0, -0.25, float("nan")):
        p = plan.copy()
        p["w"][1] = bad
        with pytest.raises(ValueError, match="weight outside"):
            check_interp_plan(p, 3)


# ---------------------------------------------------------------------------------------------------------------------- the restatement
def test_reference_at_half_is_torch_half_sum_bit_for_bit():
    from boosting_nerv_amd.hnerv_utils import embed_expand_reference, interp_plan
    g = torch.Generator().manual_seed(11)
    src = torch.randn(3, 2304, generator=g)
    _, plan = interp_plan(5, "1_1_2")
    out = embed_expand_reference(src.numpy(), plan)
    assert out.dtype == np.float32 and out.shape == (5, 2304)
    for t, (a, b) in ((1, (0, 1)), (3, (1, 2))):
        assert np.array_equal(out[t].view(np.uint32), (0.5 * (src[a] + src[b])).numpy().view(np.uint32))
    for k, t in enumerate((0, 2, 4)):
        assert np.array_equal(out[t].view(np.uint32), src[k].numpy().view(np.uint32))


def test_reference_general_weight_rounds_every_operation():
    from boosting_nerv_amd.hnerv_utils import embed_expand_reference, interp_plan
    g = torch.Generator().manual_seed(12)
    src = torch.randn(2, 4, 3, 5, generator=g)             # trailing dimensions are kept
    _, plan = interp_plan(5, "1_1_3")
    out = embed_expand_reference(src.numpy(), plan)
    assert out.shape == (5, 4, 3, 5)
    for t in (1, 2):
        w = torch.tensor(plan["w"][t])
        want = (torch.tensor(1.0) - w) * src[0] + w * src[1]            # torch fp32: a product, a product, a sum
        assert np.array_equal(out[t].view(np.uint32), want.numpy().view(np.uint32))
    assert np.array_equal(out[4], src[1].numpy()) and np.array_equal(out[3], src[1].numpy()) and np.array_equal(out[0], src[0].numpy())


# ---------------------------------------------------------------------------------------------------------------------- the flag
_CLI = "--data_path synthetic:5x180x320 --vid tiny --crop_list 180_320 --outf t -e 1"


def test_flag_is_off_by_default_and_parses():
    from boosting_nerv_amd import train_nerv_all as T
    assert T.parse_args((_CLI + " --model HNeRV").split()).embed_inter_stored is False
    a = T.parse_args((_CLI + " --model HNeRV --interpolation --data_split 1_1_2 --embed_inter_stored").split())
    assert a.embed_inter_stored is True and a.embed_inter is False
    assert T.parse_args((_CLI + " --model HNeRV_Boost --interpolation --embed_inter_stored").split()).embed_inter_stored is True
    b = T.parse_args((_CLI + " --model HNeRV --interpolation --data_split 1_1_2 --embed_inter").split())      # as ever
    assert b.embed_inter is True and b.embed_inter_stored is False


def test_flag_refusals_at_parse_time():
    from boosting_nerv_amd import train_nerv_all as T
    with pytest.raises(ValueError, match="--embed_inter_stored: the held-out frames it derives are those of an --interpolation run"):
        T.parse_args((_CLI + " --model HNeRV --embed_inter_stored").split())
    with pytest.raises(ValueError, match="--embed_inter_stored stands in place of --embed_inter"):
        T.parse_args((_CLI + " --model HNeRV --interpolation --embed_inter --embed_inter_stored").split())
    with pytest.raises(ValueError, match="--embed_inter_stored: --model NeRV_Boost has no frame embeddings"):
        T.parse_args((_CLI + " --model NeRV_Boost --interpolation --embed_inter_stored").split())
    with pytest.raises(ValueError, match="--embed_inter_stored: --shuffle_data"):
        T.parse_args((_CLI + " --model HNeRV --interpolation --embed_inter_stored --shuffle_data").split())


def test_check_posthoc_flags_admits_the_flag_and_still_refuses_embed_inter():
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    for extra in ("", " --bitstream_sparse", " --bitstream_temporal"):
        a = T.parse_args((_CLI + " --model HNeRV --interpolation --data_split 1_1_2 --embed_inter_stored --bitstream t.bin" + extra).split())
        codec.check_posthoc_flags(a)
    b = T.parse_args((_CLI + " --model HNeRV --interpolation --data_split 1_1_2 --embed_inter --bitstream t.bnrq").split())
    with pytest.raises(NotImplementedError, match="--interpolation --embed_inter scores the held-out frames from fp32 encoder outputs"):
        codec.check_posthoc_flags(b)
    with pytest.raises(ValueError, match="--yuv_loss"):                                           # the other pinned refusal of --embed_inter
        T.parse_args((_CLI + " --model HNeRV --interpolation --embed_inter --yuv_loss 1.0").split())


# ---------------------------------------------------------------------------------------------------------------------- the header key
def _parent_blob(fmt, settings, section):
    """The bytes the containers frame a payload in, restated: prefix (magic, version, payload length), JSON header with sorted keys, the
    section, CRC32 of the payload."""
    header = json.dumps(settings, sort_keys=True, separators=(",", ":")).encode("utf-8")
    payload = struct.pack("<I", len(header)) + header + b"".join(section)
    return struct.pack("<4sIQ", fmt.MAGIC, fmt.VERSION, len(payload)) + payload + struct.pack("<I", zlib.crc32(payload) & 0xFFFFFFFF)


@pytest.mark.parametrize("sparse", [False, True], ids=["qstream", "zstream"])
def test_header_key_round_trip_qstream_zstream(sparse):
    from boosting_nerv_amd import codec
    settings, lengths, records, words, fmt = PC.tensor_section(sparse)
    settings.update(full_data_length=5, embed_shape=[3, 4, 12, 12])
    plain = fmt.to_bytes(settings, lengths, records, words)
    assert plain == _parent_blob(fmt, settings, fmt._section(lengths, records, words))            # without the key: the bytes as ever
    assert "n_stored_frames" not in fmt.info(plain) and "embed_stored" not in fmt.read(plain).settings
    keyed = fmt.to_bytes(dict(settings, embed_stored=[5, 1, 1, 2]), lengths, records, words)
    back = fmt.read(keyed)
    assert back.settings["embed_stored"] == [5, 1, 1, 2] and back.settings["embed_shape"] == [3, 4, 12, 12]
    assert np.array_equal(back.words, words) and len(back.records) == len(records)
    b = fmt.info(keyed)
    assert b["n_stored_frames"] == 3 and b["total"] == 8 * len(keyed) == sum(b[k] for k in fmt.ITEMS)
    assert codec.info(keyed) == b and "the embeddings of 3 stored frames" in codec.describe_any(b)
    a = fmt.info(plain)
    assert {k: b[k] for k in fmt.ITEMS if k != "header"} == {k: a[k] for k in fmt.ITEMS if k != "header"}      # the key costs header bits only
    assert b["header"] - a["header"] == 8 * len(',"embed_stored":[5,1,1,2]')
    rest = {k: v for k, v in b.items() if k != "n_stored_frames"}
    assert codec.describe_any(rest) + "; interpolation: the embeddings of 3 stored frames, every other frame derived from them" == codec.describe_any(b)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_header_key_round_trip_pstream(sparse):
    from boosting_nerv_amd import codec, pstream
    q = PC.walk_clip(3)                                    # the three stored frames of a five-frame clip, chained in stored order
    plain, settings, e = PC.file_of(q, sparse)
    _, lengths, records, words, fmt = PC.tensor_section(sparse)
    assert plain == _parent_blob(pstream, settings, fmt._section(lengths, records, words) + pstream._embed_section(e))
    assert "n_stored_frames" not in pstream.info(plain)
    keyed_settings = dict(settings, full_data_length=5, embed_stored=[5, 1, 1, 2])
    keyed = pstream.to_bytes(keyed_settings, lengths, records, words, e)
    back = pstream.read(keyed)
    assert back.settings["embed_stored"] == [5, 1, 1, 2] and tuple(back.embeds.shape) == (3,) + PC.SHAPE
    assert np.array_equal(pstream.decode_embeds(back), q)
    b = pstream.info(keyed)
    assert b["n_stored_frames"] == 3 and b["n_embed_symbols"] == 3 * PC.P and b["total"] == 8 * len(keyed) == sum(b[k] for k in pstream.ITEMS)
    assert codec.info(keyed) == b and "the embeddings of 3 stored frames" in codec.describe_any(b)


def test_info_refuses_a_key_without_an_embedding_shape():
    from boosting_nerv_amd import qstream
    settings, lengths, records, words, fmt = PC.tensor_section(False)
    with pytest.raises(ValueError, match="embed_stored"):
        qstream.info(qstream.to_bytes(dict(settings, embed_stored=[5, 1, 1, 2]), lengths, records, words))
