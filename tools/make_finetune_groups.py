#!/usr/bin/env python3
"""Generate tests/golden/g11_finetune_groups.json from the REAL reference: the membership of the 22 parameter groups of its
surgical fine-tuning (finetune.py's get_parameter_groups), as state_dict keys of the CSwinUnet wrapper on the tiny config.

Run once in the build container (the only place /root/reference exists):

    python tools/make_finetune_groups.py

finetune.py is imported with everything it imports beside torch stubbed (loguru, torchvision, and its own networks, trainer,
config, utils and datasets modules: none of them is used by get_parameter_groups, which only walks attributes of
model.cswin_unet).  The function is applied to THIS package's model, whose attributes and state_dict keys are the reference's
(tests/test_abi.py), and every returned parameter is named by identity.  Nothing from the reference is copied: only names (data)
are stored."""
import importlib.util
import json
import os
import sys
import types
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "g11_finetune_groups.json")
STUBBED = ("loguru", "networks", "networks.vision_transformer", "trainer", "config", "utils", "torchvision", "torchvision.transforms",
           "datasets", "datasets.dataset_synapse")


def reference_get_parameter_groups():
    stubs = {}
    for name in STUBBED:
        m = types.ModuleType(name)
        m.__getattr__ = lambda attr: mock.MagicMock(name=attr)          # whatever finetune.py imports from it
        m.__path__ = []
        stubs[name] = m
    with mock.patch.dict(sys.modules, stubs):
        spec = importlib.util.spec_from_file_location("reference_finetune", os.path.join(REF, "finetune.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    return mod.get_parameter_groups


def main():
    from cswin_unet_amd.config import get_config
    from cswin_unet_amd.networks.vision_transformer import CSwinUnet
    cfg = get_config(os.path.join(ROOT, "configs", "cswin_tiny_224_lite.yaml"))
    model = CSwinUnet(cfg, img_size=224, num_classes=9)
    names = {id(p): n for n, p in model.named_parameters()}
    assert list(names.values()) == list(model.state_dict())              # no buffers: the parameter names are the keys
    groups = reference_get_parameter_groups()(model, 0)
    out = {"source": "finetune.py get_parameter_groups (:77-114), imported and applied to the tiny config's CSwinUnet",
           "groups": {g: [names[id(p)] for p in params] for g, params in groups.items()}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"{OUT}: {len(out['groups'])} groups, {sum(len(v) for v in out['groups'].values())} names, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
