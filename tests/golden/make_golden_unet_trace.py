"""Write tests/golden/unet_trace.txt: the C-ABI launch trace of the UNet host path (tests/test_gpu_unet_trace.py, which owns the recorder, the inputs
and the variants).  Run on an MI355X with the built library, on the commit whose behaviour is to be pinned:

    python tests/golden/make_golden_unet_trace.py

The file holds one `<variant> <calls> <sha256>` line per variant, the sha256 of the default variant's second noise prediction, and the default
variant's trace in full (the others would not fit the size limit of a committed file; a mismatch there is located by diffing two runs of this script).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_unet_trace as T  # noqa: E402


def main(path=T.GOLDEN):
    traces, eps_sha = T.record_variants()
    with open(path, "w") as f:
        f.write("# written by tests/golden/make_golden_unet_trace.py -- do not edit\n")
        for name, lines in traces.items():
            f.write(f"{name} {len(lines)} {T.digest(lines)}\n")
        f.write(f"eps_sha256 {eps_sha}\n--- default\n")
        f.write("\n".join(traces["default"]) + "\n")
    print(open(path).read().split("--- default")[0])


if __name__ == "__main__":
    main(*sys.argv[1:2])
