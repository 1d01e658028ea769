"""`execute.prove` refuses a witness that does not fit the circuit BEFORE it loads the SRS, the key or the plan for it, and leaves the
caller's report as it was: no device is needed to be told so (the key and SRS paths here do not exist)."""
import json
import os

import pytest

import fixture_k6 as FX


def _prove(X, witness, tmp_path, **kw):
    return X.prove(str(witness), os.path.join(FX.G, "model_k6.compiled"), str(tmp_path / "no.key"), str(tmp_path / "proof.json"), str(tmp_path / "no.srs"), **kw)


def test_a_witness_of_the_wrong_shape_is_refused_before_anything_is_loaded(tmp_path):
    from ezkl_amd import execute as X
    w = json.load(open(os.path.join(FX.G, "witness_k6.json")))
    w["inputs"][0] = w["inputs"][0][:2]
    (tmp_path / "short.json").write_text(json.dumps(w))
    report = {"kept": 1}
    with pytest.raises(ValueError, match="input shape"):
        _prove(X, tmp_path / "short.json", tmp_path, report=report)
    assert report == {"kept": 1}
    with pytest.raises(ValueError, match="synthesis must be"):
        _prove(X, tmp_path / "short.json", tmp_path, synthesis="gpu")
    with pytest.raises(OSError):                                                # a fitting witness goes on to the key, which is not there
        _prove(X, os.path.join(FX.G, "witness_k6.json"), tmp_path, report=report)
    assert report == {"kept": 1}


def test_an_input_beyond_int64_is_refused_by_name_under_synthesis_device(tmp_path):
    from ezkl_amd import codecs, execute as X
    w = json.load(open(os.path.join(FX.G, "witness_k6.json")))
    w["inputs"][0][0] = codecs.felt_to_hex_le(1 << 64)
    (tmp_path / "wide.json").write_text(json.dumps(w))
    with pytest.raises(ValueError, match="an input does not fit int64$"):
        _prove(X, tmp_path / "wide.json", tmp_path, synthesis="device")
    with pytest.raises(OSError):                                                # "auto" and "host" take such an input to the host layout
        _prove(X, tmp_path / "wide.json", tmp_path, synthesis="host")
