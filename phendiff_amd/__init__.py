"""phendiff_amd -- MI355X-native engine for PhenDiff's diffusion hot path.

Drop-in (Python-level) replacements for the objects the reference's loops drive:
``CustomCondUNet2DModel`` (``src/cond_unet_2d``), ``DDIMScheduler`` / ``DDIMInverseScheduler`` (diffusers),
``ConditionalDDIMPipeline`` (``src/pipeline_conditional_ddim``), and the DDIB class-transfer loops of
``src/utils_Img2Img.py``.  All device work goes through ``libphendiff_hip.so`` (``include/phendiff_hip.h``).
"""
from ._lib import PhenDiffHipError, lib  # noqa: F401
from .unet import CustomCondUNet2DModel, UNet2DOutput  # noqa: F401
from .schedulers import DDIMScheduler, DDIMInverseScheduler, quantile_rank  # noqa: F401
from .schedulers import DPMSolverMultistepScheduler, DPMSolverMultistepInverseScheduler  # noqa: F401
from .schedulers import GuidanceRescale, guidance_rescale  # noqa: F401
from .pipeline import ConditionalDDIMPipeline, ImagePipelineOutput  # noqa: F401
from .img2img import (inversion, ddib, inverted_regeneration, classifier_free_guidance_forward_start,  # noqa: F401
                      shard_batches, swap_binary_labels, custom_guided_generation,
                      linear_interp_custom_guidance_inverted_start, encode_to_latents, decode_to_images, LDM_preprocess, tensor_to_PIL,
                      tiled_inversion, tiled_ddib, tiled_inverted_regeneration, TiledTransferOutput)
from .noise import DeviceNoise  # noqa: F401
from .trajectories import DDIBGraph, CFGForwardStartGraph, SDDDIBGraph, GuidedTransferGraph, SDGuidedTransferGraph, TiledDDIBGraph  # noqa: F401
from .trajectories import GenerationGraph  # noqa: F401
from .masked import (class_contrast_mask, mask_blend, masked_ddib, MaskedDDIBGraph, MaskedTransferOutput, blend_state_index,  # noqa: F401
                     encode_timestep, check_mask, ContrastMask)
from . import mask_ops  # noqa: F401
from .mask_ops import (mask_distance, mask_dilate, mask_erode, mask_open, mask_close, mask_components, remove_small_components,  # noqa: F401
                       fill_holes, MaskRefine, refine_mask, disc_r2)
from . import objects  # noqa: F401
from .objects import label_objects, measure_intensity, ObjectMeasure, ObjectLabels, object_change, measure_transfer  # noqa: F401
from .tiling import TileGrid  # noqa: F401
from . import tiling  # noqa: F401
from .configs import UNET_CONFIGS, SCHEDULER_CONFIGS, SD15_UNET_CONFIG  # noqa: F401
from . import configs  # noqa: F401
from . import diagnostics  # noqa: F401
from .diagnostics import check_gaussianity, sample_distances, normaltest_from_moments, GaussianityReport  # noqa: F401
from .diagnostics import sample_ssim, ssim_maps_means, gaussian_window  # noqa: F401
from .comm import NativeComm  # noqa: F401
from . import training  # noqa: F401
from .training import DeviceTrainingSampler  # noqa: F401
from .unet_train import UNetTrainer, UNetTrainPlan, training_param_order  # noqa: F401
from . import train_state  # noqa: F401
from . import eval_generation  # noqa: F401
from .sd_unet import SDUNet2DConditionModel, CustomEmbedding, class_emb_to_encoder_hidden_states, SD21_UNET_CONFIG  # noqa: F401
from .vae import AutoencoderKL, VaeImageProcessor, DiagonalGaussianDistribution, SD_VAE_CONFIG  # noqa: F401
from .sd_pipeline import CustomStableDiffusionImg2ImgPipeline, hack_class_embedding  # noqa: F401
from .sd_unet_train import SDUNetTrainer, SDUNetTrainPlan, sd_training_param_order, sd_training_layout  # noqa: F401
from .vae_train import VaeEncodeTrainPlan, vae_training_param_order  # noqa: F401
from . import metrics  # noqa: F401,E402  (FID / IS / KID, precision / recall, density / coverage: InceptionV3Features, calculate_metrics, class_metrics_hook, precision_recall_device, density_coverage_device)
from . import data  # noqa: F401,E402  (uint8 images -> the engine's input: ImagePreprocessor, resample_tables, draw_flips)
from .data import ImagePreprocessor, band_percentiles, resample_tables_f64, restore_bands16  # noqa: F401,E402
