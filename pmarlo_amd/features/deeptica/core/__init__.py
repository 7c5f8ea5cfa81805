from .history import vamp2_proxy
from .inputs import FeaturePrep, prepare_features
from .pairs import PairInfo, build_pair_info
from .trainer_api import _estimate_top_eigenvalues, estimate_top_eigenvalues

__all__ = ["FeaturePrep", "PairInfo", "_estimate_top_eigenvalues", "build_pair_info", "estimate_top_eigenvalues",
           "prepare_features", "vamp2_proxy"]
