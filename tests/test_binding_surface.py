"""The Python binding's public surface and the C calls its Renderer wrappers make, held to tests/golden/binding_surface.json
(tests/binding_pin.py describes the snapshot and rewrites it: python tests/binding_pin.py --write).  No GPU: the surface is read
off the loaded package, and the calls are made against a stand-in for the library that records them."""
import json

import binding_pin as pin


def _golden():
    with open(pin.FIXTURE) as f:
        return json.load(f)


def _plain(v):
    return json.loads(json.dumps(v))


def test_public_surface_is_the_pinned_one(pkg):
    want, got = _golden()["surface"], _plain(pin.surface(pkg))
    assert sorted(got) == sorted(want), "public names of the package"
    for name in want:
        if want[name]["kind"] == "class":
            assert sorted(got[name]["members"]) == sorted(want[name]["members"]), "public members of %s" % name
            for m in want[name]["members"]:
                assert got[name]["members"][m] == want[name]["members"][m], "%s.%s" % (name, m)
        assert got[name] == want[name], name


def test_abi_types_are_the_pinned_ones(pkg):
    want, got = _golden()["abi"], _plain(pin.abi(pkg))
    assert sorted(got) == sorted(want) == sorted(pkg.ABI_SYMBOLS)
    for s in want:
        assert got[s] == want[s], s


def test_script_calls_every_renderer_method_that_takes_no_cuda_tensor(pkg, monkeypatch):
    fake = pin.Recorder()
    monkeypatch.setattr(pkg, "_lib", fake)
    assert pin.scripted_methods(pin.calls(pkg, fake)) == pin.public_methods(pkg) - pin.NOT_SCRIPTED


def test_c_calls_are_the_pinned_ones(pkg, monkeypatch):
    """symbol choice, argument order, NULL-ness, scalar mapping and the shapes handed to C, and what each wrapper returns"""
    fake = pin.Recorder()
    monkeypatch.setattr(pkg, "_lib", fake)
    want, got = _golden()["calls"], _plain(pin.calls(pkg, fake))
    assert [s["call"] for s in got] == [s["call"] for s in want]
    for i, (g, w) in enumerate(zip(got, want)):
        where = "step %d: %s(%s)" % (i, w["call"], ", ".join("%s=%s" % kv for kv in w["given"].items()))
        assert g["given"] == w["given"], where
        assert g.get("raised") == w.get("raised"), where
        assert g["abi"] == w["abi"], where
        assert g.get("returned") == w.get("returned"), where


def test_fixture_regenerates_byte_for_byte(pkg, monkeypatch):
    with open(pin.FIXTURE) as f:
        text = f.read()
    assert pin.dumps(pin.snapshot(pkg, lambda fake: monkeypatch.setattr(pkg, "_lib", fake))) == text
