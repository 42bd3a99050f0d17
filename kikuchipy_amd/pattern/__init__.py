from kikuchipy_amd.pattern._pattern import (  # noqa: F401
    adaptive_histogram_equalization,
    adaptive_histogram_equalization_stack,
    downsample_stack,
    fft_filter_stack,
    fft_frequency_vectors,
    get_dynamic_background,
    get_dynamic_background_stack,
    get_image_quality,
    normalize_intensity,
    normalize_intensity_stack,
    reduce_stack,
    region_sums,
    remove_dynamic_background,
    remove_static_background,
    rescale_intensity,
    rescale_intensity_stack,
)
from kikuchipy_amd.pattern._neighbours import (  # noqa: F401
    average_neighbour_dot_product_map,
    average_neighbour_patterns_stack,
    neighbour_dot_product_matrices,
)
from kikuchipy_amd.pattern._decomposition import (  # noqa: F401
    LearningResults,
    decomposition_model_stack,
    decomposition_stack,
)
