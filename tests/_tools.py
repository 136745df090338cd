"""How the tests reach the scripts they use as libraries (tools/*.py, bench.py, ...): plain helper, no fixtures."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script(relpath):
    """The script at relpath (from the repository root) as a fresh module object on every call; never put into sys.modules, so
    module-level state such as gpu_check.RESULTS is each caller's own."""
    spec = importlib.util.spec_from_file_location(os.path.splitext(os.path.basename(relpath))[0], os.path.join(ROOT, relpath))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m
