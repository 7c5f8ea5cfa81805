"""pmarlo.conformations on the MI355X engine: representative frames of conformational states,
trajectory-bootstrap error bars, kinetic importance scores, source / sink detection, transition path theory with
its dominant pathways, and find_conformations, which drives them all."""
from .finder import find_conformations  # noqa: F401
from .kinetic_importance import KineticImportanceScore, KISResult  # noqa: F401
from .results import Conformation, ConformationSet, TPTResult  # noqa: F401
from .state_detection import StateDetector  # noqa: F401
from .tpt_analysis import PATHWAY_MAX_ITERATIONS, TPTAnalysis  # noqa: F401
from .representative_picker import (  # noqa: F401
    FrameIndexLookup,
    RepresentativeFrame,
    RepresentativePicker,
    TrajectoryFrameLocator,
    TrajectorySegment,
    build_frame_index_lookup,
)
from .uncertainty import UncertaintyQuantifier, UncertaintyResult  # noqa: F401
