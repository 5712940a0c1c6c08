"""Mint tests/golden/configs/: copies of five of the reference's settings files and, as JSON, what the reference's own
``load_config`` (the unmodified src/config.py:10-59) makes of them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_config.py REFERENCE_ROOT

src/config.py is executed as it stands; only the package it imports beside yaml (``src.conv_onet``, the model builders, which
``load_config`` does not touch) is replaced by an empty module, so that nothing but PyYAML is needed."""
import importlib.util
import json
import os
import shutil
import sys
import types

FILES = ("nice_slam.yaml", "Replica/replica.yaml", "Replica/room0.yaml", "TUM_RGBD/tum.yaml", "TUM_RGBD/freiburg1_desk.yaml")
# (config, default_path) as run.py calls it (run.py:24: always with the default file)
CASES = {"nice_slam": ("nice_slam.yaml", None), "replica": ("Replica/replica.yaml", "nice_slam.yaml"),
         "room0": ("Replica/room0.yaml", "nice_slam.yaml"), "tum": ("TUM_RGBD/tum.yaml", "nice_slam.yaml"),
         "freiburg1_desk": ("TUM_RGBD/freiburg1_desk.yaml", "nice_slam.yaml"), "room0_no_default": ("Replica/room0.yaml", None)}


def main():
    ref = os.path.abspath(sys.argv[1])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
    pkg = types.ModuleType("src")
    pkg.__path__ = []
    pkg.conv_onet = types.ModuleType("src.conv_onet")
    sys.modules["src"], sys.modules["src.conv_onet"] = pkg, pkg.conv_onet
    spec = importlib.util.spec_from_file_location("src.config", os.path.join(ref, "src", "config.py"))
    config = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(config)
    for f in FILES:
        os.makedirs(os.path.dirname(os.path.join(out, f)), exist_ok=True)
        shutil.copyfile(os.path.join(ref, "configs", f), os.path.join(out, f))
    os.chdir(ref)                                  # inherit_from names paths from the reference's root
    merged = {}
    for name, (path, default) in CASES.items():
        merged[name] = {"config": path, "default": default,
                        "cfg": config.load_config(os.path.join("configs", path), None if default is None else os.path.join("configs", default))}
    with open(os.path.join(out, "merged.json"), "w") as fh:
        json.dump(merged, fh, indent=1, sort_keys=True)
    print("wrote", len(FILES), "settings files and", len(merged), "merged dicts to", out)


if __name__ == "__main__":
    main()
