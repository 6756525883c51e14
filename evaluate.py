"""Evaluate a relit video: `python evaluate.py --output_dir <run output directory> [--eval_cost] [--raft PATH] [--clip PATH] [--pick PATH] [--lpips PATH --lpips_lin PATH] [--light [--light_path JSON]]` (the reference's evaluate.py).

Reads `<output_dir>/config.yaml`, the relit video (output_opt / output, .mp4 or .avi, else output.npy) and the source video (output_gt), computes
warp-error-ssim on the device (tc_light_amd/evaluate.py: RAFT flows of the source frames, cubic warp, forward-backward mask, SSIM) and writes
`<output_dir>/result.txt` in the reference's format, one block per prompt of `generation.prompt` (the file keeps the last one, as the reference's
does).  --eval_cost adds the run's cost figures (z_*).  RAFT weights: `models.raft` of the config or --raft; a missing file is an error unless
`models.allow_random` / TCL_ALLOW_RANDOM_WEIGHTS=1 allows seeded stand-ins.  clip-frame and clip-text are computed when a CLIP ViT-B/32 checkpoint is
named (`models.clip` or --clip, OpenAI's ViT-B-32.pt or a transformers .safetensors; tokenizer directory: --clip_tokenizer, else
`models.clip_tokenizer`, else `models.text_encoder`); clip-text differs per prompt.  pick-score is computed when a PickScore_v1 checkpoint is named
(`models.pick` or --pick: a transformers snapshot directory or a .safetensors / .bin file; tokenizer directory: --pick_tokenizer, else
`models.pick_tokenizer`, else the snapshot itself, else the CLIP one); it differs per prompt too.  Figures whose checkpoint is not named are listed as
not computed; with both named result.txt holds the reference's four figures.  frame-lpips, the LPIPS-VGG distance of every relit frame but the last to
its source frame (the reference's FrameLPIPS, which its evaluate.py ships but never calls), is added when a torchvision VGG-16 state dict is named
(`models.lpips_vgg` or --lpips) together with LPIPS's linear layers (`models.lpips_lin` or --lpips_lin: the lpips package's weights/v0.1/vgg.pth);
without them nothing of it is loaded and the output is unchanged.  --light adds light-contrast and light-follow (this project's own: the mean
cosine between the light direction fitted to every relit frame and the one the run asked for -- generation.light_path, else the side of
generation.init_latent or of an fbc generation.bg_source ramp; --light_path "[[0,0],[1,180]]" overrides the config, for runs made without one) and
writes the per-frame table to `<output_dir>/light_follow.json`; without --light nothing changes.
"""
import argparse
import json
import os
import sys

import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--output_dir", type=str, default="workdir")
    ap.add_argument("--eval_cost", action="store_true")
    ap.add_argument("--raft", type=str, default=None, help="RAFT checkpoint (raft-things.pth); default: models.raft of config.yaml")
    ap.add_argument("--clip", type=str, default=None, help="CLIP ViT-B/32 checkpoint (ViT-B-32.pt); default: models.clip of config.yaml; none: no CLIP figures")
    ap.add_argument("--clip_tokenizer", type=str, default=None, help="CLIP tokenizer directory; default: models.clip_tokenizer, else models.text_encoder")
    ap.add_argument("--pick", type=str, default=None, help="PickScore_v1 checkpoint (snapshot directory or .safetensors); default: models.pick; none: no pick-score")
    ap.add_argument("--pick_tokenizer", type=str, default=None, help="tokenizer directory for pick-score; default: models.pick_tokenizer, else the snapshot, else the CLIP one")
    ap.add_argument("--lpips", type=str, default=None, help="torchvision VGG-16 state dict (.pth / .safetensors) for frame-lpips; default: models.lpips_vgg; none: no frame-lpips")
    ap.add_argument("--lpips_lin", type=str, default=None, help="LPIPS linear layers (the lpips package's weights/v0.1/vgg.pth); default: models.lpips_lin")
    ap.add_argument("--light", action="store_true", help="add light-follow / light-contrast and write light_follow.json")
    ap.add_argument("--light_path", type=str, default=None, help='keyframes [[pos, angle_deg], ...] as JSON, e.g. "[[0,0],[1,180]]"; default: the config\'s '
                    "generation.light_path, else its init_latent / bg_source side (only with --light)")
    ap.add_argument("--batch", type=int, default=4, help="frame pairs per RAFT / metric batch")
    a = ap.parse_args(argv)

    import torch
    from tc_light_amd.config_utils import _wrap
    from tc_light_amd.evaluate import (clip_frame, clip_settings, clip_text, cost_scores, find_videos, format_results, frame_lpips, light_follow,
                                       lpips_settings, not_computed, pick_score, pick_settings, read_video_u8, video_name, warp_ssim)
    from tc_light_amd.lightfit import wanted_angles
    from tc_light_amd.model_utils import allow_random, load_clip_state, load_lpips_state, load_pick_state, load_raft_state
    from tc_light_amd.raft import RAFTEngine

    with open(os.path.join(a.output_dir, "config.yaml")) as f:
        config = _wrap(yaml.safe_load(f) or {})
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate.py runs its metric on the GPU and found none")
    models = config.get("models") or {}
    edit_path, source_path = find_videos(a.output_dir)
    edit, source = read_video_u8(edit_path), read_video_u8(source_path)
    if a.light_path is not None and not a.light:
        raise ValueError("--light_path is read only with --light")
    # refused here, before a model is loaded: a config that names no light direction, or keyframes that are not a path
    wanted = wanted_angles(config, len(edit), None if a.light_path is None else json.loads(a.light_path)) if a.light else None
    print(f"[INFO] edit {edit_path} ({tuple(edit.shape)}), source {source_path} ({tuple(source.shape)})")
    clip_path, tok_dir = clip_settings(models, a.clip, a.clip_tokenizer)
    pick_path, pick_tok_dir = pick_settings(models, a.pick, a.pick_tokenizer)
    lpips_path, lpips_lin = lpips_settings(models, a.lpips, a.lpips_lin)
    left_out = not_computed(bool(clip_path), bool(pick_path))
    if left_out and pick_path:
        print(f"[INFO] not computed here: {', '.join(left_out)} (no CLIP checkpoint is configured: models.clip / --clip)")
    elif left_out and clip_path:
        print(f"[INFO] not computed here: {', '.join(left_out)} (its PickScore model is not part of this project)")
    elif left_out:
        print(f"[INFO] not computed here: {', '.join(left_out)} (their CLIP / PickScore models are not part of this project)")
    engine = RAFTEngine(load_raft_state(a.raft or models.get("raft"), allow=allow_random(models)), "cuda")
    score, _ = warp_ssim(edit, source, engine, batch=a.batch)
    scores = {"warp-error-ssim": score}
    del engine
    prompts = ((config.get("generation") or {}).get("prompt") or {})
    prompts = (list(prompts.values()) if isinstance(prompts, dict) else [prompts]) or [""]
    per_prompt = [{} for _ in prompts]
    if clip_path:
        from tc_light_amd.clip import CLIPEngine, load_tokenizer
        clip_engine = CLIPEngine(load_clip_state(clip_path, allow=allow_random(models)), "cuda")
        tokenizer = load_tokenizer(tok_dir)
        feats = clip_engine.encode_image(edit)
        scores["clip-frame"] = clip_frame(edit, clip_engine, features=feats)
        for extra, prompt in zip(per_prompt, prompts):
            extra["clip-text"] = clip_text(edit, prompt, clip_engine, tokenizer, allow_random=allow_random(models), features=feats)
        del clip_engine, feats                                              # freed before the larger PickScore engine is built
        torch.cuda.empty_cache()
    if pick_path:
        from tc_light_amd.clip import load_tokenizer, pick_engine
        state, pick_config = load_pick_state(pick_path, allow=allow_random(models))
        pick_eng = pick_engine(state, "cuda", pick_config)
        del state
        tokenizer = load_tokenizer(pick_tok_dir)
        feats = pick_eng.encode_image(edit)                                 # once; every prompt reuses them
        for extra, prompt in zip(per_prompt, prompts):
            extra["pick-score"] = pick_score(edit, prompt, pick_eng, tokenizer, allow_random=allow_random(models), features=feats)
        del pick_eng, feats
    if lpips_path:
        from tc_light_amd.lpips import LPIPSEngine
        torch.cuda.empty_cache()
        lpips_eng = LPIPSEngine(load_lpips_state(lpips_path, lpips_lin, allow=allow_random(models)), "cuda")
        scores["frame-lpips"], _ = frame_lpips(edit, source, lpips_eng, batch=a.batch)
        del lpips_eng
    if a.light:
        scores["light-follow"], scores["light-contrast"], frames = light_follow(edit, source, wanted, "cuda")
        with open(os.path.join(a.output_dir, "light_follow.json"), "w") as f:
            json.dump(frames, f, indent=1)
    if a.eval_cost:
        scores.update(cost_scores(config, edit.shape[2], edit.shape[1]))
    name = video_name(config)
    for extra, prompt in zip(per_prompt, prompts):
        scores.update(extra)
        text = format_results(name, prompt, scores)
        with open(os.path.join(a.output_dir, "result.txt"), "w") as f:
            f.write(text)
        print(text)
    return scores


if __name__ == "__main__":
    main()
