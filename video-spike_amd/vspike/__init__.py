"""vspike — MI355X-native (gfx950) video->spike training hot path of PPWangyc/video-spike.

Drop-in surface (src/utils/utils.py:28-34 of the reference): `NAME2MODEL[config.model.model_class]`
builds the plugin from `config.model`; `forward(inputs) -> log-rates (B, 100, N)`.  All compute
runs in libvspike.so (hand-written HIP, include/vspike.h) — there is no CPU fallback.
"""
from .behaviour import behaviour_rrr_data, flow_features, get_rrr_data
from .contrast import ContrastViT
from .config import DictConfig, config_from_kwargs, load_run_config, update_config
from .linear import Linear
from .mae import MAE
from .loss import InfoNCE, MSEMeanLoss, PoissonNLLMeanLoss, make_criterion, mse_mean, poisson_nll_mean
from .optim import FusedAdamW
from .pca import PCA, pca_embedding, pca_rrr_data
from .r3d import R3D
from .rrr import RRR, RRRGD, PixelFeatures, pixel_rrr_data, prepare_rrr_inputs, train_rrr, train_rrr_baseline
from .temporal import VideoMAETemporal
from .vit import VideoMAE

NAME2MODEL = {
    "Linear": Linear,
    "VideoMAE": VideoMAE,
    # BASELINE C4's CNN encoder (no reference counterpart: SURVEY.md section 0), same plugin surface
    "R3D": R3D,
    # BASELINE C5's encoder + temporal transformer stage (no reference counterpart either: DESIGN.md section 7)
    "VideoMAETemporal": VideoMAETemporal,
    # the reference's contrastive pretraining model (src/model/vit_mae/vit_mae.py:26-44, `pretrain.py --model c`)
    "ContrastViT": ContrastViT,
    # the reference's masked-autoencoder pretraining model (vit_mae.py:45-94, `pretrain.py --model m`)
    "MAE": MAE,
}

__all__ = ["NAME2MODEL", "Linear", "VideoMAE", "VideoMAETemporal", "R3D", "ContrastViT", "MAE", "InfoNCE", "RRR", "train_rrr", "RRRGD", "prepare_rrr_inputs", "train_rrr_baseline", "PixelFeatures", "pixel_rrr_data", "PCA", "pca_embedding", "pca_rrr_data", "flow_features", "get_rrr_data", "behaviour_rrr_data", "FusedAdamW", "poisson_nll_mean", "PoissonNLLMeanLoss",
           "mse_mean", "MSEMeanLoss", "make_criterion",
           "DictConfig", "update_config", "config_from_kwargs", "load_run_config"]
