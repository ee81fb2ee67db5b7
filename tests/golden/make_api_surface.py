#!/usr/bin/env python3
"""Regenerates tests/golden/api_surface.json: what `import fdeflate_amd` offers, name by name.

    python tests/golden/make_api_surface.py

For every name in fdeflate_amd.__all__: a function's signature, a class's public methods with their signatures, a
constant's value.  tests/test_api_surface.py compares the tree under test with the file; regenerate it only when the
public surface is meant to change.  Needs neither the built library nor a GPU.
"""
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def api_surface():
    import fdeflate_amd as fd
    surface = {}
    for name in fd.__all__:
        obj = getattr(fd, name)
        if inspect.isclass(obj):
            methods = {"__init__": obj.__init__}
            methods.update((k, v) for k, v in vars(obj).items() if inspect.isfunction(v) and not k.startswith("_"))
            surface[name] = {"class": {k: str(inspect.signature(v)) for k, v in sorted(methods.items())}}
        elif callable(obj):
            surface[name] = {"function": str(inspect.signature(obj))}
        else:
            surface[name] = {"constant": json.loads(json.dumps(obj))}
    return surface


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(os.path.join(HERE, "api_surface.json"), "w") as f:
        json.dump(api_surface(), f, indent=1, sort_keys=True)
        f.write("\n")
