"""How the tests reach the scripts they use as libraries (tools/*.py, bench.py, ...) and the yardstick the scoring tests share: plain
helpers, no fixtures."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script(relpath):
    """The script at relpath (from the repository root) as a fresh module object on every call; never put into sys.modules, so
    module-level state such as gpu_check.RESULTS is each caller's own."""
    spec = importlib.util.spec_from_file_location(os.path.splitext(os.path.basename(relpath))[0], os.path.join(ROOT, relpath))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    """The bit patterns of a float32 or float64 tensor."""
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint64 if t.element_size() == 8 else np.uint32)


def rel_err(x, ref):
    """max|x - ref| / max|ref| in float64."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


MARGIN = 8.0


def _yardstick(what, dev, f32, f64, floor=0.0):
    """e(device) <= 8 e(float32 reference), the latter counted as at least `floor`; prints the ratio before it asserts."""
    e_dev, e_ref = rel_err(dev, f64), max(rel_err(f32, f64), floor)
    print(f'\n{what}: e(device) {e_dev:.3e}  e(float32 reference) {e_ref:.3e}  ratio {e_dev / e_ref if e_ref else float("inf"):.3f}')
    assert e_dev <= MARGIN * e_ref, (what, e_dev, e_ref)
