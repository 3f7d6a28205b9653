"""Writes `reference_config_keys.json`: the `sac_config` / `replay_config` keys of the reference's default and
per-environment YAML files (including the per-agent override sections, `ma_config`), per file, for
`tests/test_plugin_surface.py::test_every_reference_config_key_is_accepted`.  Only the key names are kept.

    python tests/golden/make_config_keys.py [REFERENCE_DIR]      (default: ref_shims.REFERENCE_ROOT)
"""
import glob
import json
import sys
from pathlib import Path

import yaml

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))


def collect(ref: Path) -> dict:
    files = sorted(glob.glob(str(ref / 'envs/**/config*.yaml'), recursive=True)) + [str(ref / 'algorithm/default_config.yaml')]
    out = {}

    def visit(node, keys):
        if not isinstance(node, dict):
            return
        for k, v in node.items():
            if k in ('sac_config', 'replay_config') and isinstance(v, dict):
                keys[k].update(v)
            visit(v, keys)

    for f in files:
        keys = {'sac_config': set(), 'replay_config': set()}
        with open(f) as fh:
            visit(yaml.safe_load(fh), keys)
        out[str(Path(f).relative_to(ref))] = {k: sorted(v) for k, v in keys.items()}
    return out


if __name__ == '__main__':
    if len(sys.argv) > 1:
        root = Path(sys.argv[1])
    else:
        from ref_shims import REFERENCE_ROOT
        root = Path(REFERENCE_ROOT)
    (HERE / 'reference_config_keys.json').write_text(json.dumps(collect(root), indent=1, sort_keys=True) + '\n')
