"""Record tests/golden/resample.npz: results of the reference's own resampling back end (preproc/resampling.py with
preproc/firws.py), both loaded by file path (they need only NumPy and SciPy; the package they import each other through
is a stub registered here).

    python tools/record_resample_golden.py <path to the reference's syncopy/preproc directory>
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (method, samplerate, resamplefs, trial length, order, lpfreq)
CASES = {
    "r600_700": ("resample", 1000.0, 600.0, 700, 700, None),
    "r600_odd": ("resample", 1000.0, 600.0, 333, 61, None),
    "r600_short": ("resample", 1000.0, 600.0, 50, 1000, None),
    "r333": ("resample", 1000.0, 333.0, 512, 512, None),
    "r441_lp": ("resample", 1000.0, 441.0, 300, 300, 100.0),
    "r999": ("resample", 1000.0, 999.0, 130, 130, None),
    "r750_lp": ("resample", 1000.0, 750.0, 129, 129, 200.0),
    "r2000_1200": ("resample", 2000.0, 1200.0, 257, 257, None),
    "r30k_1k": ("resample", 30000.0, 1000.0, 3000, 1000, None),
    "d250": ("downsample", 1000.0, 250.0, 203, None, None),
}
NCHAN = 2


def _load(folder):
    pkg = types.ModuleType("syncopy")
    sub = types.ModuleType("syncopy.preproc")
    pkg.preproc = sub
    sys.modules["syncopy"], sys.modules["syncopy.preproc"] = pkg, sub
    mods = {}
    for name in ("firws", "resampling"):
        spec = importlib.util.spec_from_file_location(f"syncopy.preproc.{name}", os.path.join(folder, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        setattr(sub, name, mod)
        mods[name] = mod
    return mods["resampling"]


def main(folder):
    ref = _load(folder)
    rng = np.random.default_rng(20261016)
    out = {"names": np.array(sorted(CASES))}
    for name, (method, fs, new_fs, n, order, lpfreq) in CASES.items():
        x = (rng.normal(size=(n, NCHAN)) + rng.normal(size=(1, NCHAN))).astype(np.float32)
        out[f"{name}_in"] = x
        out[f"{name}_par"] = np.array([fs, new_fs, -1 if order is None else order, -1 if lpfreq is None else lpfreq])
        if method == "resample":
            y = ref.resample(x, fs, new_fs, lpfreq=lpfreq, order=order)
        else:
            y = ref.downsample(x, fs, new_fs)
        out[f"{name}_out"] = np.asarray(y, dtype=np.float32)          # what the reference's routine stores
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "resample.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
