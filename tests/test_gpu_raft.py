"""GPU: RAFT (data.flow_model: raft) against the reference RAFT run on the CPU (tests/golden/raft.npz, tests/golden/make_golden_raft.py) with the
seeded weights of tc_light_amd.raft.seeded_state_dict: the encoders in both input conventions, forward(test_mode=True, iters=20) at two sizes,
the load_flow raft branch; the fused SepConvGRU half-steps and convf1 against torch's f32 convolutions; the batched driver against per-pair calls."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda"


@pytest.fixture(scope="module")
def G(golden):
    return golden("raft")


@pytest.fixture(scope="module")
def eng(dev, G):
    from tc_light_amd.raft import RAFTEngine, seeded_state_dict
    return RAFTEngine(seeded_state_dict(int(G["seed"])), dev)


def test_encoders_vs_reference(eng, G, dev):
    img = torch.from_numpy(G["enc_img_u8"]).float() / 255.0
    for conv, scale in (("01", 1.0), ("255", 255.0)):
        x = (2 * (img * scale / 255.0) - 1.0).to(dev)
        fm, c, (h, w) = eng.encode(x)
        for name, got in (("fnet", fm), ("cnet", c)):
            ref = torch.from_numpy(G[f"{name}_{conv}"]).float()
            got = got.float().view(1, h, w, 256).permute(0, 3, 1, 2)
            r = rel(got, ref)
            print(f"{name} [{conv}] rel-L2 {r:.2e}")
            assert r <= 5e-3, (name, conv, r)


def test_forward_vs_reference(eng, G, dev):
    for H, W in ((128, 192), (144, 256)):
        pair = torch.from_numpy(G["clip_u8"][:2] if H == 128 else G[f"pair_{H}x{W}_u8"]).float() / 255.0
        for conv, scale in (("01", 1.0), ("255", 255.0)):
            low, up = eng.forward(pair[0:1] * scale, pair[1:2] * scale, iters=20)
            rl, ru = rel(low, torch.from_numpy(G[f"low_{H}x{W}_{conv}"]).float()), rel(up[..., ::2, ::2], torch.from_numpy(G[f"up_{H}x{W}_{conv}"]).float())
            print(f"forward {H}x{W} [{conv}]: flow_low rel-L2 {rl:.2e}, flow_up rel-L2 {ru:.2e}")
            assert tuple(up.shape) == (1, 2, H, W) and tuple(low.shape) == (1, 2, H // 8, W // 8)
            assert rl <= 1.5e-2 and ru <= 1.5e-2, (H, W, conv, rl, ru)


def _sep_ref(x, w, b, vertical):
    return F.conv2d(x, w, b, padding=(2, 0) if vertical else (0, 2))


def test_fused_gru_half_steps_vs_torch(eng, dev):
    """Both half-steps at 90x160, B = 2, with the context fold: z, r*h and the blended h against f32 convolutions of the same f16 inputs."""
    g = torch.Generator().manual_seed(4)
    B, h, w = 2, 90, 160
    P = B * h * w
    net = torch.tanh(torch.randn(B, 128, h, w, generator=g)).half()
    inp = torch.relu(torch.randn(B, 128, h, w, generator=g)).half()
    mot = torch.relu(torch.randn(B, 128, h, w, generator=g)).half()
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(P, 128).contiguous().to(dev)
    from tc_light_amd.raft import seeded_state_dict
    sd = seeded_state_dict(5)
    fold = eng.context_fold(rows(inp), B, h, w)
    for di, dn in ((0, "1"), (1, "2")):
        wz, wr, wq = (sd[f"update_block.gru.conv{k}{dn}.weight"].half().float() for k in "zrq")
        bz, br, bq = (sd[f"update_block.gru.conv{k}{dn}.bias"] for k in "zrq")
        hx = torch.cat([net, inp, mot], 1).float()
        z_ref = torch.sigmoid(_sep_ref(hx, wz, bz, di))
        r_ref = torch.sigmoid(_sep_ref(hx, wr, br, di))
        rh_ref = r_ref * net.float()
        q_ref = torch.tanh(_sep_ref(torch.cat([rh_ref.half().float(), inp.float(), mot.float()], 1), wq, bq, di))   # q conv on the f16 r*h the kernel sees
        h_ref = (1 - z_ref) * net.float() + z_ref * q_ref
        hn = rows(net)
        z = torch.empty(P, 128, dtype=torch.float32, device=dev); rh = torch.empty(P, 128, dtype=torch.float16, device=dev)
        eng.gru_half(di, hn, rows(mot), fold[di], z, rh, B, h, w)
        torch.cuda.synchronize()
        back = lambda t: t.float().view(B, h, w, 128).permute(0, 3, 1, 2)
        rz, rrh, rhh = rel(back(z), z_ref), rel(back(rh), rh_ref), rel(back(hn), h_ref)
        print(f"GRU half {dn}: z {rz:.2e}, r*h {rrh:.2e}, h {rhh:.2e}")
        assert rz <= 2e-3 and rrh <= 2e-3 and rhh <= 2e-3, (dn, rz, rrh, rhh)


def test_convf1_vs_torch(eng, dev):
    from tc_light_amd.lib import lib, stream
    from tc_light_amd.raft import seeded_state_dict
    sd = seeded_state_dict(5)
    g = torch.Generator().manual_seed(6)
    B, h, w = 2, 90, 160
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    c0 = torch.stack([xs, ys])[None].expand(B, 2, h, w)
    c1 = (c0 + 3 * torch.randn(B, 2, h, w, generator=g)).contiguous()
    ref = torch.relu(F.conv2d(c1 - c0, sd["update_block.encoder.convf1.weight"], sd["update_block.encoder.convf1.bias"], padding=3))
    y = torch.empty(B * h * w, 128, dtype=torch.float16, device=dev)
    lib().tcl_raft_convf1_f16(c1.to(dev), eng.convf1[0], eng.convf1[1], y, 128, B, h, w, stream())
    r = rel(y.float().view(B, h, w, 128).permute(0, 3, 1, 2), ref)
    print(f"convf1 rel-L2 {r:.2e}")
    assert r <= 2e-3


def test_estimate_flows_vs_load_flow(eng, G, dev):
    from tc_light_amd.raft import estimate_flows_raft
    clip = (torch.from_numpy(G["clip_u8"]).float() / 255.0).to(dev)
    fut, past = estimate_flows_raft(eng, clip, batch=4)
    rf, rp = torch.from_numpy(G["load_flow_future"]).float(), torch.from_numpy(G["load_flow_past"]).float()
    assert tuple(fut.shape) == tuple(past.shape) == (4, 2, 128, 192)
    assert fut[-1].abs().max().item() == 0 and past[0].abs().max().item() == 0
    fut, past = fut[..., ::2, ::2], past[..., ::2, ::2]                   # the fixture keeps every other pixel
    for i in range(3):
        a, b = rel(fut[i], rf[i]), rel(past[i + 1], rp[i + 1])
        print(f"load_flow pair {i}: future {a:.2e}, past {b:.2e}")
        assert a <= 1.5e-2 and b <= 1.5e-2


def test_batched_driver_vs_per_pair(eng, dev):
    from tc_light_amd.raft import estimate_flows_raft
    g = torch.Generator().manual_seed(8)
    base = F.interpolate(torch.rand(1, 3, 20, 28, generator=g), size=(160, 224), mode="bicubic", align_corners=False).clamp(0, 1)
    frames = torch.cat([base[:, :, 2 * i:2 * i + 128, 3 * i:3 * i + 192] for i in range(5)]).to(dev)
    fut, past = estimate_flows_raft(eng, frames, batch=4)
    fut2, past2 = estimate_flows_raft(eng, frames, batch=4)
    assert torch.equal(fut, fut2) and torch.equal(past, past2)            # deterministic
    for i in range(4):
        _, up = eng.forward(frames[i:i + 1], frames[i + 1:i + 2], iters=20)    # [0, 1] frames as the raft branch passes them
        _, upb = eng.forward(frames[i + 1:i + 2], frames[i:i + 1], iters=20)
        assert rel(fut[i], up[0]) <= 1e-3 and rel(past[i + 1], upb[0]) <= 1e-3


def test_full_size_pair(eng, dev):
    g = torch.Generator().manual_seed(9)
    a = torch.rand(1, 3, 720, 1280, generator=g) * 255
    b = torch.roll(a, (3, 5), (2, 3))
    low, up = eng.forward(a, b, iters=20)
    low2, up2 = eng.forward(a, b, iters=20)
    assert tuple(low.shape) == (1, 2, 90, 160) and tuple(up.shape) == (1, 2, 720, 1280)
    assert torch.isfinite(up).all() and torch.isfinite(low).all()
    assert torch.equal(up, up2) and torch.equal(low, low2)
