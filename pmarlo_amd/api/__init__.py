"""pmarlo.api operators on the MI355X engine (the slice the MSM path uses)."""
from .features import (  # noqa: F401
    align_trajectory,
    compute_features,
    compute_universal_embedding,
    compute_universal_metric,
    feature_cache_file,
    trig_expand_periodic,
)
