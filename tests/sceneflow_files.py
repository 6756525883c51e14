"""Writers of the SceneFlow file formats for the tests, independent of the readers in tc_light_amd/sceneflow.py."""
import struct

import numpy as np


def write_pfm(path, a, little=True, scale=1.0):
    """The format, written independently of the reader: tag, 'W H', signed scale, rows bottom to top."""
    a = np.asarray(a, np.float32)
    ch = 3 if a.ndim == 3 else 1
    h, w = a.shape[:2]
    with open(path, "wb") as f:
        f.write(b"PF\n" if ch == 3 else b"Pf\n")
        f.write(f"{w} {h}\n".encode())
        f.write(f"{-scale if little else scale:f}\n".encode())
        for y in range(h - 1, -1, -1):
            row = a[y].reshape(-1)
            f.write(struct.pack(("<" if little else ">") + f"{row.size}f", *row.tolist()))


def cam_text(frames):
    out = []
    for fid, L, R in frames:
        out += [f"Frame {fid}", "L " + " ".join(repr(float(v)) for v in L.reshape(-1)), "R " + " ".join(repr(float(v)) for v in R.reshape(-1)), ""]
    return "\n".join(out) + "\n"
