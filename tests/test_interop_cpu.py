"""CPU, build container only: the reference loads checkpoint + replay files written by the product
(`tests/golden/product_ckpt/`, see `tests/golden/ref_load_product.py`).  Skipped where `/root/reference` does not
exist (the GPU box)."""
import importlib.util
import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent


def _reference_readable() -> bool:
    """the reference checkout `golden/ref_shims.py` names is there and this user may read it (a location that cannot be
    read counts as absent rather than failing the collection)"""
    spec = importlib.util.spec_from_file_location('_ref_shims_location', HERE / 'golden' / 'ref_shims.py')
    shims = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shims)
    return os.path.isfile(os.path.join(shims.REFERENCE_ROOT, 'algorithm', 'sac_base.py'))


@pytest.mark.skipif(not _reference_readable(), reason='needs the reference checkout (present and readable)')
@pytest.mark.skipif(not (HERE / 'golden' / 'product_ckpt' / '3.pth').exists(), reason='product files not generated yet')
def test_reference_restores_product_written_files():
    r = subprocess.run([sys.executable, str(HERE / 'golden' / 'ref_load_product.py')], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'reference restored the product files: ok' in r.stdout
