"""The public surface of the package is pinned by tests/golden/api_surface.json: the names of fdeflate_amd.__all__, every
function's signature, every class's public methods, every constant's value (tests/golden/make_api_surface.py writes
the file and says when to).  fdeflate_amd.api lists the names once and the package takes them from there."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maker():
    spec = importlib.util.spec_from_file_location("make_api_surface", os.path.join(ROOT, "tests", "golden", "make_api_surface.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_public_surface_is_the_recorded_one(golden_dir):
    import fdeflate_amd as fd
    from fdeflate_amd import api
    with open(os.path.join(golden_dir, "api_surface.json")) as f:
        recorded = json.load(f)
    assert len(recorded) == 100 and len(fd.__all__) == len(set(fd.__all__)) == 100
    assert set(fd.__all__) == set(recorded)
    assert fd.__all__ is api.__all__
    surface = _maker().api_surface()
    for name in recorded:
        assert surface[name] == recorded[name], name
        assert getattr(fd, name) is getattr(api, name), name
    # the A / B and debug flags stay out of the package but within reach
    assert api.FLAG_NO_LANES == 32 and "FLAG_NO_LANES" not in fd.__all__ and not hasattr(fd, "FLAG_NO_LANES")
