"""Shared by tests/test_container_cpu.py: one small file of every kind, built through the public API and the case
helpers of the other suites, the damages a reader must refuse (or take) with the very words it had before the kinds shared one container
layer, and record(), which wrote tests/golden/containers/ from the package as it was BEFORE that layer.  The fixtures are a recording of
that commit: record() is never run against the code under test."""
import hashlib
import importlib
import io
import json
import os
import struct
import sys
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "containers")
MODULES = dict(bnrv="bitstream", bnrc="rstream", bnre="estream", bnrw_gaussian="wstream", bnrw_empirical="wstream", bnrt="tstream", bnrq="qstream",
               bnrz="zstream", bnrp_dense="pstream", bnrp_sparse="pstream")
NAMES = tuple(MODULES)
FRAMING_DAMAGES = ("empty", "first_15_bytes", "other_magic", "version_2", "last_byte_removed", "one_byte_appended", "payload_bit_flipped")


def module_of(name):
    return importlib.import_module("boosting_nerv_amd." + MODULES[name])


def build():
    """-> {name: bytes}, in the order of NAMES.  Deterministic across processes."""
    import pstream_cases
    import tstream_cases
    from boosting_nerv_amd import codec
    v1 = tstream_cases.version1_blob(tstream_cases.walk())

    def repacked(**kinds):
        out = io.BytesIO()
        codec.repack(v1, out, run=64, **kinds)
        return out.getvalue()

    def section(sparse):
        settings, lengths, records, words, fmt = pstream_cases.tensor_section(sparse)
        return fmt.to_bytes(settings, lengths, records, words)

    files = dict(bnrv=v1, bnrc=repacked(), bnre=repacked(tables="empirical"), bnrw_gaussian=repacked(wide=True),
                 bnrw_empirical=repacked(tables="empirical", wide=True), bnrt=repacked(wide=True, temporal=True), bnrq=section(False), bnrz=section(True),
                 bnrp_dense=pstream_cases.file_of(pstream_cases.walk_clip(4), False)[0], bnrp_sparse=pstream_cases.file_of(pstream_cases.walk_clip(4), True)[0])
    assert tuple(files) == NAMES
    return files


def _reframed(blob, payload):
    """`payload` in the framing of `blob`, the CRC computed here: the parser is reached, not the CRC check."""
    return blob[:8] + struct.pack("<Q", len(payload)) + payload + struct.pack("<I", zlib.crc32(payload) & 0xFFFFFFFF)


def _with_header(blob, header):
    payload = blob[16:-4]
    n, = struct.unpack_from("<I", payload)
    return _reframed(blob, struct.pack("<I", len(header)) + header + payload[4 + n:])


def _header_end(blob):
    return 16 + 4 + struct.unpack_from("<I", blob, 16)[0]


DAMAGES = {
    "empty": lambda b: b"",
    "first_15_bytes": lambda b: b[:15],
    "other_magic": lambda b: (b"BNRC" if b[:4] == b"BNRV" else b"BNRV") + b[4:],
    "version_2": lambda b: b[:4] + struct.pack("<I", 2) + b[8:],
    "last_byte_removed": lambda b: b[:-1],
    "one_byte_appended": lambda b: b + b"\0",
    "payload_bit_flipped": lambda b: b[:len(b) // 2] + bytes([b[len(b) // 2] ^ 0x10]) + b[len(b) // 2 + 1:],
    # ---- with the CRC recomputed
    "header_is_a_list": lambda b: _with_header(b, b"[]"),
    "header_is_not_utf8": lambda b: _with_header(b, b"\xff"),
    "header_length_is_2_to_the_32_minus_1": lambda b: _reframed(b, b"\xff\xff\xff\xff" + b[20:-4]),
    "payload_ends_behind_the_header": lambda b: _reframed(b, b[16:_header_end(b)]),
    "four_zero_bytes_appended_to_the_payload": lambda b: _reframed(b, b[16:-4] + b"\0\0\0\0"),
}
assert tuple(DAMAGES)[:7] == FRAMING_DAMAGES and len(DAMAGES) == 12


def digest(stream):
    """SHA-256 of repr() of what read() returned, every array printed in full."""
    with np.printoptions(threshold=sys.maxsize):
        return hashlib.sha256(repr(stream).encode()).hexdigest()


def outcome(fmt, damaged):
    """What a reader makes of a damaged file -> {"error": the whole message | None, "digest": None | digest of what it read}."""
    try:
        stream = fmt.read(damaged)
    except ValueError as e:
        return {"error": str(e), "digest": None}
    return {"error": None, "digest": digest(stream)}


def observed(name, blob):
    """Everything the fixtures pin about one file, from the package as it is imported now."""
    from boosting_nerv_amd import codec
    fmt = module_of(name)
    return {"info": [[k, v] for k, v in fmt.info(blob).items()], "codec_info": [[k, v] for k, v in codec.info(blob).items()],
            "describe": codec.describe_any(codec.info(blob)), "damages": {d: outcome(fmt, damage(blob)) for d, damage in DAMAGES.items()}}


def record(directory=GOLDEN):
    """Write the ten files and expected.json.  Run with the package of the commit before the container layer on the path, never again."""
    os.makedirs(directory, exist_ok=True)
    expected = {}
    for name, blob in build().items():
        with open(os.path.join(directory, name + ".bin"), "wb") as f:
            f.write(blob)
        expected[name] = observed(name, blob)
    with open(os.path.join(directory, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1, sort_keys=False)
        f.write("\n")
    return expected
