#!/usr/bin/env python3
"""Generates tests/golden/ref_train_settings.json: the ``optimizer`` / ``lr_scheduler`` / ``training_steps`` settings of the
reference's four configs, read with ``sgcdet_amd.mmcv_lite.Config.fromfile``.  Settings only (dicts, numbers, strings): what
``sgcdet_amd.optim.build_optimizer`` takes, so that tests/test_optim_cpu.py does not need the reference checkout.

    python tests/golden/make_golden_train_settings.py <reference checkout>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_configs import NAMES, encode  # noqa: E402  (also puts the repository root on sys.path)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "configs")):
        sys.exit("usage: make_golden_train_settings.py <reference checkout holding configs/>")
    from sgcdet_amd.mmcv_lite import Config
    out = {}
    for n in NAMES:
        cfg = Config.fromfile(os.path.join(sys.argv[1], "configs", n + ".py"))
        out[n] = {k: encode(cfg[k]) for k in ("optimizer", "lr_scheduler", "training_steps")}
    with open(os.path.join(HERE, "ref_train_settings.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
