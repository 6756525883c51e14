"""SceneFlowDataParser (reference: utils/dataparsers/sceneflow_dataparsers.py:215-369): FlyingThings3D / Driving / Monkaa-style trees with
ground-truth disparity, optical flow and camera poses -> frames, flows, soft masks and the SPATIO-TEMPORAL Unique Video Tensor ids.

Layout under data.data_dir (scene_path = <15mm|35mm>_focallength/scene_<backwards|forwards>/<fast|slow>, stereo_sel = left | right):
  frames_cleanpass/<scene_path>/<stereo>/%04d.png
  disparity/<scene_path>/<stereo>/%04d.pfm
  optical_flow/<scene_path>/into_{future,past}/<stereo>/OpticalFlowInto{Future,Past}_%04d_{L,R}.pfm
  camera_data/<scene_path>/camera_data.txt
Host I/O is written from the file formats: PNG through PIL; PFM = 'PF' (3 channels) or 'Pf' (1 channel), 'width height', a scale whose sign
gives the byte order (negative: little endian), then float32 rows stored BOTTOM TO TOP; camera_data.txt = blocks of 'Frame n', an 'L' line and
an 'R' line of 16 numbers each (camera-to-world, row major), a blank line.
Unprojection, per-track means, quantisation and the unique-rows step run on the device (tc_light_amd/voxel.py, csrc/voxel.hip).
"""
import os

import numpy as np
import torch

from .dataparser import process_frames
from .flow_ids import get_flowid, get_soft_mask_bwds
from .voxel import unproject_sceneflow, voxelization

FOCAL = ("15mm_focallength", "35mm_focallength")
DIRECTION = ("scene_backwards", "scene_forwards")
SPEED = ("fast", "slow")
STEREO = ("left", "right")


def read_pfm(path):
    """-> (float32 array [H,W] ('Pf') or [H,W,3] ('PF') with row 0 at the TOP, scale)."""
    with open(path, "rb") as f:
        tag = f.readline().strip()
        if tag not in (b"PF", b"Pf"):
            raise ValueError(f"{path}: not a PFM file (header {tag!r})")
        dims = f.readline().split()
        while len(dims) < 2:                             # width and height may sit on two lines
            dims += f.readline().split()
        w, h = int(dims[0]), int(dims[1])
        scale = float(f.readline().strip())
        ch = 3 if tag == b"PF" else 1
        raw = f.read(w * h * ch * 4)
    if len(raw) != w * h * ch * 4:
        raise ValueError(f"{path}: truncated PFM ({len(raw)} of {w * h * ch * 4} bytes)")
    a = np.frombuffer(raw, dtype="<f4" if scale < 0 else ">f4").astype(np.float32)
    a = a.reshape((h, w, 3) if ch == 3 else (h, w))[::-1]
    return np.ascontiguousarray(a), abs(scale)


def read_camera_data(path):
    """camera_data.txt -> [{'frame_id': n, 'left': [4,4] f64, 'right': [4,4] f64}, ...] in file order."""
    out, cur = [], None
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            t = line.split()
            if not t:
                continue
            if t[0] == "Frame":
                cur = {"frame_id": int(t[1])}
                out.append(cur)
            elif t[0] in ("L", "R") and cur is not None:
                if len(t) != 17:
                    raise ValueError(f"{path}:{ln}: expected 16 numbers after {t[0]!r}, got {len(t) - 1}")
                cur["left" if t[0] == "L" else "right"] = np.array(t[1:], dtype=np.float64).reshape(4, 4)
            else:
                raise ValueError(f"{path}:{ln}: unexpected line {line.strip()!r}")
    for c in out:
        if "left" not in c or "right" not in c:
            raise ValueError(f"{path}: frame {c['frame_id']} lacks an L or an R line")
    return out


class SceneFlowDataParser:
    def __init__(self, data_config, device):
        g = data_config.get
        self.data_dir = g("data_dir", "data/sceneflow")
        self.scene_path = g("scene_path", "15mm_focallength/scene_backwards/fast")
        self.stereo_sel = g("stereo_sel", "left")
        self.voxel_size = g("voxel_size", None)
        self.contract = g("contract", False)
        self.use_raft = g("use_raft", False)
        self.fps = g("fps", 30)
        self.alpha = g("alpha", 0.1)
        self.h, self.w = int(data_config["height"]), int(data_config["width"])
        self.device = device
        self.unq_inv = None
        if self.stereo_sel not in STEREO:
            raise ValueError(f"data.stereo_sel must be one of {STEREO}, got {self.stereo_sel!r}")
        sp = str(self.scene_path).split("/")
        if len(sp) != 3 or sp[0] not in FOCAL or sp[1] not in DIRECTION or sp[2] not in SPEED:
            raise ValueError(f"data.scene_path must be <{'|'.join(FOCAL)}>/<{'|'.join(DIRECTION)}>/<{'|'.join(SPEED)}>, got {self.scene_path!r}")
        j = os.path.join
        self.rgb_path = j(self.data_dir, "frames_cleanpass", self.scene_path, self.stereo_sel)
        self.disparity_path = j(self.data_dir, "disparity", self.scene_path, self.stereo_sel)
        self.future_flow_path = j(self.data_dir, "optical_flow", self.scene_path, "into_future", self.stereo_sel)
        self.past_flow_path = j(self.data_dir, "optical_flow", self.scene_path, "into_past", self.stereo_sel)
        self.camera_path = j(self.data_dir, "camera_data", self.scene_path, "camera_data.txt")
        f = 450.0 if "15mm" in self.scene_path else 1050.0       # the two fixed intrinsics (fx, fy, cx, cy)
        self.intrinsics = (f, f, 479.5, 269.5)
        self._cam = None

    @property
    def cam_info(self):
        if self._cam is None:
            self._cam = read_camera_data(self.camera_path)
        return self._cam

    @property
    def n_frames(self):
        return len(self.cam_info)

    def _read_rgbs(self, frame_ids):
        from PIL import Image
        out = []
        for i in frame_ids:
            p = os.path.join(self.rgb_path, f"{self.cam_info[i]['frame_id']:04d}.png")
            out.append(torch.from_numpy(np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8).copy()).permute(2, 0, 1))
        return torch.stack(out).float() / 255.0

    def load_video(self, frame_ids=None, path=None):
        """frames [N,3,h,w] f32 in [0,1] on the device (sceneflow_dataparsers.py:276-286); `path` reads another clip (the background video)
        the way the video parser does."""
        if path is not None:
            from .dataparser import VideoDataParser
            return VideoDataParser({"rgb_path": path, "height": self.h, "width": self.w}, self.device).load_video(path=path)
        ids = list(frame_ids) if frame_ids is not None else list(range(self.n_frames))
        return process_frames(self._read_rgbs(ids), self.h, self.w).to(self.device)

    def load_gt_flows(self, frame_ids, src_hw):
        """The into_future / into_past PFMs: first two channels, process_frames, scaled by max(w/W, h/H) of the SOURCE size (W, H) so that the
        vectors are in working-size pixels.  (The reference takes that factor after the resize, where it is 1: sceneflow_dataparsers.py:361-366.)"""
        tag = "L" if self.stereo_sel == "left" else "R"
        fut, past = [], []
        for i in frame_ids:
            fid = self.cam_info[i]["frame_id"]
            for lst, d, name in ((fut, self.future_flow_path, "Future"), (past, self.past_flow_path, "Past")):
                a, _ = read_pfm(os.path.join(d, f"OpticalFlowInto{name}_{fid:04d}_{tag}.pfm"))
                if a.ndim != 3:
                    raise ValueError(f"flow PFM for frame {fid} has one channel")
                lst.append(torch.from_numpy(a[..., :2].copy()).permute(2, 0, 1))
        H, W = src_hw
        s = max(self.w / W, self.h / H)
        return tuple((process_frames(torch.stack(t), self.h, self.w) * s).contiguous().to(self.device) for t in (fut, past))

    @torch.no_grad()
    def load_data(self, frame_ids=None, models=None, allow_random=False, rgb_threshold=0.01):
        """sceneflow_dataparsers.py:289-321 -> dict(frames, flows, past_flows, masks, inv, k, p_world, flow_ids, n_tracks).

        Depth = fx / disparity is computed in float64 and rounded to float32 once (the reference's own result depends on the NumPy version's
        scalar promotion: a float32 quotient under NumPy 2, a float64 one rounded by torch.tensor under NumPy 1).  Unprojection, the means,
        the quantisation and the unique-rows step run on the device.  use_raft routes the processed frames through estimate_flows_raft (its
        size rules apply); otherwise the ground-truth flows are read."""
        ids = list(frame_ids) if frame_ids is not None else list(range(self.n_frames))
        rgbs = self._read_rgbs(ids)
        depths, c2ws = [], []
        for i in ids:
            disp, _ = read_pfm(os.path.join(self.disparity_path, f"{self.cam_info[i]['frame_id']:04d}.pfm"))
            if disp.ndim == 3:
                disp = disp[..., 0]
            with np.errstate(divide="ignore"):
                depths.append(torch.from_numpy((self.intrinsics[0] / disp.astype(np.float64)).astype(np.float32)))
            c2ws.append(torch.from_numpy(self.cam_info[i][self.stereo_sel].astype(np.float32)))
        depth = torch.stack(depths).contiguous().to(self.device)
        c2w = torch.stack(c2ws).contiguous().to(self.device)
        n, _, H, W = rgbs.shape
        if tuple(depth.shape) != (n, H, W):
            raise ValueError(f"disparity maps {tuple(depth.shape[1:])} do not match the frames {(H, W)}")
        p_world = process_frames(unproject_sceneflow(depth, self.intrinsics, c2w), self.h, self.w).contiguous()
        frames = process_frames(rgbs, self.h, self.w).contiguous().to(self.device)
        if self.use_raft:
            from .model_utils import load_raft_state
            from .raft import RAFTEngine, estimate_flows_raft
            engine = RAFTEngine(load_raft_state((models or {}).get("raft"), allow=allow_random), self.device)
            flows, past = estimate_flows_raft(engine, frames)
        else:
            flows, past = self.load_gt_flows(ids, (H, W))
        masks = get_soft_mask_bwds(frames, flows, past, alpha=self.alpha)
        flow_ids, n_tracks = get_flowid(frames, flows, masks, rgb_threshold)
        inv, k = voxelization(flow_ids, frames, p_world, self.voxel_size, n, self.h, self.w, contract=self.contract)
        self.unq_inv = inv
        return dict(frames=frames, flows=flows, past_flows=past, masks=masks, inv=inv, k=k, p_world=p_world, flow_ids=flow_ids, n_tracks=n_tracks)
