"""The host Vorbis decoder after its packet-level code moved into csrc/vorbis_core.hpp returns
exactly what it returned before: tests/golden/vorbis_host_hashes.json was written by
tests/golden/make_vorbis_hashes.py against a build of the commit before the move (SHA-256 of the
decoded samples with rate and length, or the error text, per named stream of
tests/vorbis_streams.py and for the real libvorbis file); the hashes are recomputed here with the
current build."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_vorbis_hashes", os.path.join(GOLDEN, "make_vorbis_hashes.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)


@pytest.fixture(scope="module")
def now():
    return mk.hashes()


def test_every_named_stream_is_in_the_golden_file_and_unchanged(now):
    want = json.load(open(os.path.join(GOLDEN, "vorbis_host_hashes.json")))
    assert sorted(now) == sorted(want)
    bad = [k for k in want if now[k] != want[k]]
    assert not bad, [(k, want[k], now[k]) for k in bad[:5]]


def test_the_golden_file_holds_decodes_and_errors():
    want = json.load(open(os.path.join(GOLDEN, "vorbis_host_hashes.json")))
    errors = [k for k, v in want.items() if v.startswith("error: ")]
    assert 0 < len(errors) < len(want) // 2
    assert not any(want[name].startswith("error") for name, _ in mk.vs.matrix())
