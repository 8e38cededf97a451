"""CPU suite (``-m "not gpu"``) of the container layer: the eight kinds of file write the bytes, give the budgets and
refuse damaged files with the words recorded in tests/golden/containers/ from the commit before they shared container.py
(container_cases.record), and the shared pieces exist once."""
import ast
import json
import os

import pytest

import container_cases as C
from conftest import ROOT

PACKAGE = os.path.join(ROOT, "boosting_nerv_amd")
NINE = ("container", "bitstream", "qstream", "zstream", "pstream", "rstream", "estream", "wstream", "tstream")
_cache = {}


def _expected():
    if not _cache:
        _cache["expected"] = json.load(open(os.path.join(C.GOLDEN, "expected.json")))
        _cache["files"] = {name: open(os.path.join(C.GOLDEN, name + ".bin"), "rb").read() for name in C.NAMES}
        _cache["built"] = C.build()
    return _cache["expected"], _cache["files"], _cache["built"]


def test_the_recording_covers_every_case_and_every_framing_damage_is_a_refusal():
    expected, files, _ = _expected()
    assert tuple(expected) == C.NAMES == tuple(files)
    for name in C.NAMES:
        assert tuple(expected[name]["damages"]) == tuple(C.DAMAGES), name
        for damage in C.FRAMING_DAMAGES:
            assert expected[name]["damages"][damage]["error"] is not None, (name, damage)
        for damage, want in expected[name]["damages"].items():
            assert (want["error"] is None) != (want["digest"] is None), (name, damage)


@pytest.mark.parametrize("name", C.NAMES)
def test_the_files_are_rebuilt_and_rewritten_byte_for_byte(name):
    _, files, built = _expected()
    fmt = C.module_of(name)
    assert built[name] == files[name]
    assert fmt.to_bytes(*fmt.read(files[name])) == files[name]


@pytest.mark.parametrize("name", C.NAMES)
def test_the_budgets_are_the_recorded_ones_in_the_recorded_order(name):
    from boosting_nerv_amd import codec
    expected, files, _ = _expected()
    fmt = C.module_of(name)
    assert [[k, v] for k, v in fmt.info(files[name]).items()] == expected[name]["info"]
    assert [[k, v] for k, v in codec.info(files[name]).items()] == expected[name]["codec_info"]
    assert codec.describe_any(codec.info(files[name])) == expected[name]["describe"]


@pytest.mark.parametrize("damage", tuple(C.DAMAGES))
@pytest.mark.parametrize("name", C.NAMES)
def test_a_damaged_file_is_refused_or_taken_as_recorded(name, damage):
    expected, files, _ = _expected()
    assert C.outcome(C.module_of(name), C.DAMAGES[damage](files[name])) == expected[name]["damages"][damage]


def test_framing_and_cursor_exist_once_and_no_message_is_renamed():
    """The CRC, the prefix struct and the cursor class live in container.py alone; none of the nine modules calls .replace() inside an
    except handler (how the kinds once renamed each other's messages)."""
    holders = {}
    for name in sorted(os.listdir(PACKAGE)):
        if name.endswith(".py"):
            text = open(os.path.join(PACKAGE, name)).read()
            for piece in ("zlib.crc32", '"<4sIQ"', "class _Cursor", "class Cursor"):
                if piece in text:
                    holders.setdefault(piece, []).append(name)
    assert holders == {piece: ["container.py"] for piece in ("zlib.crc32", '"<4sIQ"', "class Cursor")}, holders
    for module in NINE:
        text = open(os.path.join(PACKAGE, module + ".py")).read()
        assert "str(e).replace(" not in text, module
        for handler in (n for n in ast.walk(ast.parse(text)) if isinstance(n, ast.ExceptHandler)):
            calls = [n for n in ast.walk(handler) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "replace"]
            assert not calls, (module, handler.lineno)
