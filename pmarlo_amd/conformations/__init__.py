"""pmarlo.conformations on the MI355X engine: representative frames of conformational states,
trajectory-bootstrap error bars and kinetic importance scores."""
from .kinetic_importance import KineticImportanceScore, KISResult  # noqa: F401
from .representative_picker import (  # noqa: F401
    FrameIndexLookup,
    RepresentativeFrame,
    RepresentativePicker,
    TrajectoryFrameLocator,
    TrajectorySegment,
    build_frame_index_lookup,
)
from .uncertainty import UncertaintyQuantifier, UncertaintyResult  # noqa: F401
