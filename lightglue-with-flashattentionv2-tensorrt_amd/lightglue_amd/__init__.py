"""MI355X-native MHAHeadDim64: the fused FlashAttention-v2 (head_dim 64) hot path of
qdLMF/LightGlue-with-FlashAttentionV2-TensorRT, as hand-written gfx950 HIP kernels behind
the reference plugin's configurePlugin()/enqueue() surface (C ABI: include/mha_hd64.h).
"""
from ._lib import LIB_PATH, LibraryMissing, load as load_library  # noqa: F401
from .plugin import (  # noqa: F401
    Attention,
    LightGlueAttentionPlugin,
    LightGlueAttentionPluginCreator,
    MHAHeadDim64,
    PluginError,
    mha_hd64,
    mha_hd64_batched,
    mha_hd64_grouped,
    set_concurrency_hint,
    set_stream_mode,
)
from . import ops  # noqa: F401,E402  (registers torch.ops.lightglue_amd.*)
from .matcher import (  # noqa: F401,E402
    AdaptiveResult,
    adaptive_reference,
    adaptive_thresholds,
    seeded_confidence_state_dict,
)
from .frontend import Features, KeypointFrontend, frontend_reference  # noqa: F401,E402
from .superpoint import (  # noqa: F401,E402
    SuperPointEncoder,
    extract_pairs,
    match_images,
    seeded_superpoint_state_dict,
    superpoint_reference,
)
from .image import (  # noqa: F401,E402
    ImageBatch,
    ImageInput,
    PreparedImages,
    image_reference,
    match_source_images,
    resample_matrix,
    target_size,
)
from .geometry import (  # noqa: F401,E402
    FundamentalRansac,
    GeometryResult,
    epipolar_error,
    fundamental_refit,
    ransac_reference,
    ransac_samples,
    solve7_reference,
    two_view_scene,
    verify_source_images,
)

__all__ = [
    "FundamentalRansac",
    "GeometryResult",
    "epipolar_error",
    "fundamental_refit",
    "ransac_reference",
    "ransac_samples",
    "solve7_reference",
    "two_view_scene",
    "verify_source_images",
    "ImageBatch",
    "ImageInput",
    "PreparedImages",
    "image_reference",
    "match_source_images",
    "resample_matrix",
    "target_size",
    "Features",
    "KeypointFrontend",
    "frontend_reference",
    "SuperPointEncoder",
    "extract_pairs",
    "match_images",
    "seeded_superpoint_state_dict",
    "superpoint_reference",
    "AdaptiveResult",
    "adaptive_reference",
    "adaptive_thresholds",
    "seeded_confidence_state_dict",
    "Attention",
    "LightGlueAttentionPlugin",
    "LightGlueAttentionPluginCreator",
    "MHAHeadDim64",
    "PluginError",
    "mha_hd64",
    "mha_hd64_batched",
    "mha_hd64_grouped",
    "set_concurrency_hint",
    "set_stream_mode",
    "load_library",
    "LIB_PATH",
]
