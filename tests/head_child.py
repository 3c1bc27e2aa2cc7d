"""Child process of tests/test_gpu_head.py, one per environment setting (the VASR_* switches are read once per process, by the
devtools build VASR_LIB_PATH names): the cases of tests/head_reference.py named on the command line through the head in f16x2
and bf16x3 -> their log-probs in the .npz given first."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
import head_reference as H  # noqa: E402


def main():
    path, names = sys.argv[1], sys.argv[2:]
    out = {}
    for n in names:
        for a, y in H.device_head(H.BY_NAME[n], torch.device("cuda:0"), ("f16x2", "bf16x3")).items():
            out[f"{n}/{a}"] = y
    np.savez(path, **out)
    print("HEAD_CHILD_OK")


if __name__ == "__main__":
    main()
