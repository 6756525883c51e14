"""invert.py surface of the reference (invert.py:325-332): python invert.py --config Y [-i video].

DDIM inversion of the source video on the IC-Light UNet (tc_light_amd/invert.py): writes `<inversion.save_path>/<model_key>/noisy_latents_<t>.pt`,
the start latents a following `run.py` picks up through `generation.latents_path` ("latent path found ...").  run.py itself never inverts on the
IC-Light path (reference run.py:13-22): invert.py first, run.py second is the workflow.

load_config -> seed_everything -> generation.use_lora (as run.py) -> init_iclight -> Inverter(pipe, scheduler, config)(config.inversion.save_path).
`Inverter(None, None, config)` -- what a caller transliterated from the reference's run.py builds -- keeps saying that iclight needs no inversion.
"""
import random
import sys

import numpy as np
import torch

from tc_light_amd.config_utils import load_config
from tc_light_amd.invert import Inverter, check_config
from tc_light_amd.model_utils import init_iclight

__all__ = ["Inverter", "main"]


def seed_everything(seed):
    torch.manual_seed(seed); torch.cuda.manual_seed_all(seed); random.seed(seed); np.random.seed(seed)


def main(argv=None):
    config = load_config(argv)
    seed_everything(config.seed)
    check_config(config)                          # every refusal comes before a model is loaded
    lora = None
    if config.generation.get("use_lora"):         # generate_utils.py:95-96, exactly as run.py: read and checked before any model is loaded
        from tc_light_amd.lora import from_config
        lora = from_config(config.generation.get("lora"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe, scheduler, config.model_key = init_iclight(dev, config.get("models") or {}, seed=config.seed, lora=lora)
    return Inverter(pipe, scheduler, config, lora=lora)(config.inversion.save_path)


if __name__ == "__main__":
    main(sys.argv[1:])
