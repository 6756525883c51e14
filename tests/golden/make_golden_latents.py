"""Generate tests/golden/latents.npz by RUNNING THE REFERENCE's own `get_latents_dir` / `load_latent` (utils/VidToMe/utils.py:200-213, 304-309) and
`VidToMeGenerator.check_latent_exists` (utils/VidToMe/generate_utils.py:323-334) on the CPU.

Needs the reference checkout (TCL_REFERENCE, default /root/reference); only the .npz and this script are committed.  The modules cannot be
imported here (diffusers / torchvision are absent), so the three functions are pulled out of the reference files with `ast` at run time and
exec'd, as make_golden_path1.py does.  They run against a real directory: the script asks the reference which file it probes (an `os.path.exists`
that records), saves a tiny latent tensor under exactly that name and lets the reference load it.

Recorded (data only): the latent tensor [7,4,2,3], the frame selection and what `load_latent` returns for it (and for frame_ids=None), the file
name for a 0-dim tensor timestep (what `scheduler.timesteps[0]` is) and for a plain int, the directory names for three model keys, and
`check_latent_exists` before and after the file is there.
"""
import ast
import os
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TCL_REFERENCE", "/root/reference")
MODEL_KEYS = ["iclight", "stablediffusionapi/realistic-vision-v51", None]
FRAME_IDS = [0, 2, 3, 6]


def _function(path, name, ns, cls=None):
    tree = ast.parse(open(path).read())
    body = tree.body
    if cls is not None:
        body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    f = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)
    f.decorator_list = []
    exec(compile(ast.Module(body=[f], type_ignores=[]), path, "exec"), ns)
    return ns[name]


def main():
    probed = []

    def exists(p):
        probed.append(p)
        return os.path.exists(p)
    rec_os = types.SimpleNamespace(path=types.SimpleNamespace(join=os.path.join, exists=exists))
    ns = {"os": rec_os, "torch": torch}
    utils = REF + "/utils/VidToMe/utils.py"
    get_latents_dir = _function(utils, "get_latents_dir", ns)
    load_latent = _function(utils, "load_latent", ns)
    check = _function(REF + "/utils/VidToMe/generate_utils.py", "check_latent_exists", ns, cls="VidToMeGenerator")

    g = np.random.default_rng(31)
    latents = torch.from_numpy(g.standard_normal((7, 4, 2, 3)).astype(np.float32))
    timesteps = torch.tensor([999, 961, 923])                 # what a scheduler's .timesteps is: an int64 tensor; [0] is 0-dim
    out = dict(latents=latents.numpy(), frame_ids=np.array(FRAME_IDS, np.int64), timesteps=timesteps.numpy())
    with tempfile.TemporaryDirectory() as root:
        dirs = [get_latents_dir(root, k) for k in MODEL_KEYS]
        out["model_keys"] = np.array(["" if k is None else k for k in MODEL_KEYS])
        out["dir_names"] = np.array([os.path.relpath(d, root) for d in dirs])
        d = dirs[0]
        os.makedirs(d)
        stub = types.SimpleNamespace(use_pnp=False, scheduler=types.SimpleNamespace(timesteps=timesteps))
        out["exists_before"] = np.array(bool(check(stub, d)))
        assert len(probed) == 1 and os.path.dirname(probed[0]) == d
        out["file_name_tensor_t"] = np.array(os.path.basename(probed[0]))
        torch.save(latents, probed[0])
        out["exists_after"] = np.array(bool(check(stub, d)))
        out["selected"] = load_latent(d, timesteps[0], frame_ids=FRAME_IDS).numpy()
        out["selected_all"] = load_latent(d, timesteps[0]).numpy()
        del probed[:]
        try:
            load_latent(d, 961)                                # a plain int timestep: only the name it probes is recorded
        except AssertionError:
            pass
        out["file_name_int_t"] = np.array(os.path.basename(probed[0]))
    np.savez_compressed(os.path.join(HERE, "latents.npz"), **out)
    for k in ("dir_names", "file_name_tensor_t", "file_name_int_t", "exists_before", "exists_after"):
        print(k, out[k])


if __name__ == "__main__":
    main()
