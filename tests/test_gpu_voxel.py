"""GPU: the spatio-temporal Unique Video Tensor kernels (csrc/voxel.hip) and tc_light_amd.voxel against the CPU references of tests/voxel_refs.py:
unique rows (partition and count equal to torch.unique(dim=0), first-appearance numbering, bit-identical across runs), per-track means (bit for
bit against a sequential scatter), voxel keys (bit for bit against torch's floor division), voxelization end to end (golden cases of the
reference and a synthetic scene) and the unprojection (rounding-error bound of its stated float sequence)."""
import numpy as np
import pytest
import torch

import synth
import voxel_refs as R

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _keys_case(name):
    g = np.random.default_rng(17)
    if name == "dup":                                    # heavy duplication: long atomicMin chains; n no multiple of any block size
        pool = g.integers(-1000, 1000, (311, 6))
        return pool[g.integers(0, 311, 50021)]
    if name == "distinct":                               # all distinct; multiplicative pattern: the low 16 bits of every key are zero
        i = np.arange(65536, dtype=np.int64)[:, None]
        k = (i * 65536 * np.arange(1, 7, dtype=np.int64)[None, :]) & 0xFFFFFFFF
        return np.where(k >= 2 ** 31, k - 2 ** 32, k)
    if name == "extremes":
        vals = np.array([I32_MIN, I32_MAX, -1, 0, 1, -5, 5, I32_MIN + 1, I32_MAX - 1], dtype=np.int64)
        return vals[g.integers(0, vals.size, (4099, 2))]
    if name == "one":
        return np.array([[42]], dtype=np.int64)
    if name == "c1":
        return g.integers(-20, 20, (257, 1))
    raise KeyError(name)


@pytest.mark.parametrize("name", ["dup", "distinct", "extremes", "one", "c1"])
def test_unique_rows(name):
    dev = _dev()
    from tc_light_amd.lib import lib, stream
    keys = torch.from_numpy(_keys_case(name).astype(np.int32))
    n, c = keys.shape
    _, want = torch.unique(keys, dim=0, return_inverse=True)
    k_want = int(want.max()) + 1
    if name == "dup":
        assert k_want == 311
    if name == "distinct":
        assert k_want == n
    L = lib()
    kd = keys.to(dev)
    nbytes = L.tcl_unique_rows_workspace_bytes(n)
    assert nbytes >= 2 * n * 4
    ws = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev)       # the header: the call clears what it needs itself
    runs = []
    for _ in range(2):                                   # the workspace is reused as the first call left it
        inv = torch.full((n,), -1, dtype=torch.int32, device=dev)
        count = torch.full((1,), -1, dtype=torch.int32, device=dev)
        L.tcl_unique_rows_i32(kd, n, c, inv, count, ws, stream())
        runs.append((inv.cpu(), int(count.item())))
    (inv, cnt), (inv2, cnt2) = runs
    assert cnt == k_want and cnt2 == k_want
    assert torch.equal(inv, inv2)                        # deterministic numbering: bit for bit
    assert np.array_equal(inv.numpy().astype(np.int64), R.canon(want))         # first appearance in row order, same partition as torch.unique


def test_unique_rows_rejects_bad_arguments():
    dev = _dev()
    from tc_light_amd.lib import lib, stream
    L = lib()
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    assert L.tcl_unique_rows_workspace_bytes(2 ** 30 + 1) == 0
    for n, c in ((0, 1), (2 ** 30 + 1, 1), (4, 0), (4, 7)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_unique_rows_i32(t, n, c, t, t, t, stream())


@pytest.fixture(scope="module")
def flow_scene():
    """N = 5, 24x40: the engine's own masks and flow ids on a translating synthetic clip (tests/synth.py frames, analytic flows)."""
    dev = _dev()
    from tc_light_amd.flow_ids import get_flowid, get_soft_mask_bwds
    n, h, w = 5, 24, 40
    d = synth.video_clip(n, h, w, seed=4, shift=(2, 1), jitter=0.0)
    fr = d["frames"].to(dev)
    past = torch.zeros(n, 2, h, w, device=dev); past[1:, 0] = 2.0; past[1:, 1] = 1.0
    fut = torch.zeros(n, 2, h, w, device=dev); fut[:-1, 0] = -2.0; fut[:-1, 1] = -1.0
    masks = get_soft_mask_bwds(fr, fut, past, alpha=0.1)
    ids, k = get_flowid(fr, fut, masks)
    assert k < n * h * w                                 # tracks persist across frames
    return dict(frames=fr, ids=ids, k=k, n=n, h=h, w=w)


@pytest.mark.parametrize("c", [1, 2, 3])
def test_track_mean_bit_parity(flow_scene, c):
    from tc_light_amd.voxel import track_mean
    s = flow_scene
    g = torch.Generator().manual_seed(c)
    vals = s["frames"].cpu() if c == 3 else (torch.randn(s["n"], c, s["h"], s["w"], generator=g) * 100.0)
    mean, cnt = track_mean(vals.to(s["frames"].device).contiguous(), s["ids"], s["k"])
    rmean, rcnt = R.track_mean_ref(vals, s["ids"].cpu(), s["k"])
    assert torch.equal(cnt.cpu(), rcnt)
    assert torch.equal(mean.cpu().view(torch.int32), rmean.view(torch.int32))


def test_track_mean_refuses_repeated_ids(flow_scene):
    from tc_light_amd.voxel import track_mean
    s = flow_scene
    ids = s["ids"].clone()
    ids[2, 0, 1] = ids[2, 0, 0]                          # one id twice inside frame 2
    with pytest.raises(ValueError):
        track_mean(s["frames"], ids, s["k"])


def test_voxel_keys_bit_parity():
    dev = _dev()
    from tc_light_amd.voxel import voxel_keys
    g = np.random.default_rng(23)
    K, vs = 20000, 0.05
    vsf, rvf = np.float32(vs), np.float32(2 / 255)
    xyz = g.uniform(-30, 30, (K, 3)).astype(np.float32)
    rgb = g.uniform(0, 1, (K, 3)).astype(np.float32)
    xyz[0] = [-31.0, -30.5, -32.25]                      # the column minimum: these coordinates equal xyz_min
    mn = xyz.min(axis=0)
    assert np.array_equal(mn, xyz[0])
    m = g.integers(0, 1200, (3000, 3)).astype(np.float32)
    mult = (mn + m * vsf).astype(np.float32)             # (close to) exact multiples of the cell size above xyz_min, and one ulp either side
    xyz[100:3100] = mult
    xyz[3100:6100] = np.nextafter(mult, np.float32(np.inf))
    xyz[6100:9100] = np.nextafter(mult, np.float32(-np.inf)).clip(mn, None)
    xyz[9100:9200, 1] = mn[1]
    rm = (g.integers(0, 128, (3000, 3)).astype(np.float32) * rvf).astype(np.float32)
    rgb[100:3100] = rm
    rgb[3100:6100] = np.nextafter(rm, np.float32(np.inf))
    rgb[6100:9100] = np.nextafter(rm, np.float32(-np.inf)).clip(0, None)
    rgb[9100:9300] = 0.0
    rgb[9300:9400] = -0.0
    rgb[9400:9500] = 1.0
    t_rgb, t_xyz, t_mn = torch.from_numpy(rgb), torch.from_numpy(xyz), torch.from_numpy(mn)
    keys = voxel_keys(t_rgb.to(dev), t_xyz.to(dev), t_mn.to(dev), vs).cpu()
    want = R.keys_ref(t_rgb, t_xyz, t_mn, vs)
    assert keys.dtype == torch.int32 and tuple(keys.shape) == (K, 6)
    assert torch.equal(keys.long(), want)
    assert (want[:, :3].min(dim=0).values == 0).all()    # the rows at xyz_min sit in cell 0


def _run_voxelization(ids, rgb, xyz, vs, inst, dev):
    from tc_light_amd.voxel import voxelization
    n, _, h, w = rgb.shape
    inv, k = voxelization(ids.to(dev), rgb.to(dev), xyz.to(dev), vs, n, h, w, instance_ids=None if inst is None else inst.to(dev))
    want = R.voxelization_ref(ids.cpu().reshape(-1), R.rows_nchw(rgb.cpu()), R.rows_nchw(xyz.cpu()), vs, None if inst is None else inst.cpu())
    assert inv.dtype == torch.int32 and inv.numel() == n * h * w
    assert k == int(want.max()) + 1 == int(inv.max().item()) + 1
    assert np.array_equal(R.canon(inv), R.canon(want))
    return inv, k, want


@pytest.mark.parametrize("case,use_voxel,use_inst", [("vox", True, False), ("vox_inst", True, True), ("inst_only", False, True)])
def test_voxelization_golden(golden, case, use_voxel, use_inst):
    dev = _dev()
    g = golden("voxel")
    ids, rgb, xyz = (torch.from_numpy(g[k]) for k in ("flow_ids", "rgb", "xyz"))
    inst = torch.from_numpy(g["instance"]) if use_inst else None
    inv, k, _ = _run_voxelization(ids, rgb, xyz, float(g["voxel_size"]) if use_voxel else None, inst, dev)
    assert np.array_equal(R.canon(inv), R.canon(g[case + "_inv"]))             # the reference's own result
    assert k == int(g[case + "_inv"].max()) + 1


def test_voxelization_synthetic_scene_and_surface():
    """N = 6, 32x48: a fronto-parallel plane with a few colour levels, translating 2 x 1 pixels a frame; world pitch 0.01 a pixel, voxels of 0.03."""
    dev = _dev()
    from tc_light_amd.flow_ids import get_flowid, get_soft_mask_bwds
    from tc_light_amd.voxel import voxelization
    n, h, w, sx, sy, pitch, vs = 6, 32, 48, 2, 1, 0.01, 0.03
    fr = (torch.floor(synth.video_clip(n, h, w, seed=5, shift=(sx, sy), jitter=0.0)["frames"] * 4) / 4 + 0.1).clamp(0, 1)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    xyz = torch.stack([torch.stack([(xs + k * sx) * pitch, (ys + k * sy) * pitch, torch.full((h, w), -3.0)]) for k in range(n)]).float()
    past = torch.zeros(n, 2, h, w); past[1:, 0] = sx; past[1:, 1] = sy
    fut = torch.zeros(n, 2, h, w); fut[:-1, 0] = -sx; fut[:-1, 1] = -sy
    frd = fr.to(dev)
    masks = get_soft_mask_bwds(frd, fut.to(dev), past.to(dev), alpha=0.1)
    ids, n_tracks = get_flowid(frd, fut.to(dev), masks)
    inv, k, want = _run_voxelization(ids.reshape(-1), fr, xyz, vs, None, dev)
    k_ref = int(want.max()) + 1
    assert 0.1 * n_tracks <= k_ref <= 0.9 * n_tracks, (k_ref, n_tracks)         # merging is really exercised
    same, k_same = voxelization(ids.reshape(-1), frd, xyz.to(dev), None, n, h, w)
    assert k_same == n_tracks and torch.equal(same, ids.reshape(-1))           # voxel_size None, no instances: the ids unchanged
    with pytest.raises(NotImplementedError):
        voxelization(ids.reshape(-1), frd, xyz.to(dev), vs, n, h, w, contract=True)


def _rigid(g):
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, g.uniform(-20, 20, 3)
    return m


def test_unproject_against_f64():
    dev = _dev()
    from tc_light_amd.voxel import unproject_sceneflow
    g = np.random.default_rng(31)
    n, h, w = 3, 20, 36
    K = (450.0, 450.0, 479.5, 269.5)
    depth = torch.from_numpy(g.uniform(0.5, 50, (n, h, w)).astype(np.float32))
    c2w = torch.from_numpy(np.stack([_rigid(g) for _ in range(n)]).astype(np.float32))
    out = unproject_sceneflow(depth.to(dev), K, c2w.to(dev)).cpu()
    ref, bound = R.unproject_ref(depth, K, c2w)
    assert tuple(out.shape) == (n, 3, h, w)
    err = (out.double() - ref).abs()
    tol = 6 * 2.0 ** -23 * bound                         # three roundings in x, four products, three sums: the gamma bound of the stated sequence
    print(f"unproject: max err {err.max().item():.3e}, max err / tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all()


def test_unproject_rejects_bad_sizes():
    dev = _dev()
    from tc_light_amd.lib import lib, stream
    t = torch.zeros(64, device=dev)
    for n, h, w in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 65536, 65536)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            lib().tcl_unproject_sceneflow(t, t, n, h, w, 450.0, 450.0, 479.5, 269.5, t, stream())
