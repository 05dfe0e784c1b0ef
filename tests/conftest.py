import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (runs via gpurun)")
    config.addinivalue_line("markers", "slow: long-running CPU test")


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    cache = {}

    def load(name):
        if name not in cache:
            # a fixture too large for one committed file continues in <name>.part<i>.npz
            # (tests/golden/make_golden.py: save_parts)
            import glob
            cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
            for part in sorted(glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part*.npz"))):
                cache[name].update(np.load(part))
        return cache[name]
    return load
