"""Child process of tests/test_gpu_sep.py and tests/test_gpu_act_f64.py, one per environment setting (the VASR_* switches are
read once per process, by the devtools build VASR_LIB_PATH names): the cases of tests/sep_reference.py named on the command
line (each with its own activation and residual mode), in f16x2 and bf16x3 -> their outputs and launch counts in the .npz
given first."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
import sep_reference as SEP  # noqa: E402


def main():
    path, names = sys.argv[1], sys.argv[2:]
    out = {}
    for n in names:
        got = SEP.device_outputs(SEP.BY_NAME[n], torch.device("cuda:0"), ("f16x2", "bf16x3"))
        for a, g in got.items():
            out[f"{n}/{a}"] = g["y"].numpy()
            out[f"{n}/{a}/counts"] = np.asarray(g["counts"])
    np.savez(path, **out)
    print("SEP_CHILD_OK")


if __name__ == "__main__":
    main()
