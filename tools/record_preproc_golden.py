"""Record tests/golden/preproc.npz: results of the reference's own windowed-sinc module (preproc/firws.py), loaded by file
path (it needs only NumPy and SciPy).

    python tools/record_preproc_golden.py <path to the reference's syncopy/preproc/firws.py>
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(path):
    spec = importlib.util.spec_from_file_location("reference_firws", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    cut = {"lp": 0.1, "hp": 0.23, "bp": np.array([0.08, 0.2]), "bs": np.array([0.045, 0.055])}
    for window in ("hamming", "hann", "blackman"):
        for order in (24, 31):
            for ftype, fc in cut.items():
                out[f"wsinc_{window}_{order}_{ftype}"] = ref.design_wsinc(window, order, fc, ftype)
    out["cut_lp"], out["cut_hp"], out["cut_bp"], out["cut_bs"] = cut["lp"], cut["hp"], cut["bp"], cut["bs"]
    kernel = ref.design_wsinc("hamming", 40, 0.1, "lp")
    out["minphase_in"] = kernel
    out["minphase_out"] = ref.minphaserceps(kernel)
    rng = np.random.default_rng(20261016)
    trial = rng.normal(size=(37, 3)).astype(np.float32)
    out["fir_trial"] = trial
    for name, order in (("short", 12), ("long", 60)):          # "long": 61 taps on 37 samples
        k = ref.design_wsinc("hann", order, 0.15, "lp")
        out[f"fir_kernel_{name}"] = k
        out[f"fir_fft_{name}"] = ref.apply_fir(trial, k, "fft")
        out[f"fir_direct_{name}"] = ref.apply_fir(trial, k, "direct")
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "preproc.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
