"""pmarlo.conformations on the MI355X engine: representative frames of conformational states and
trajectory-bootstrap error bars."""
from .representative_picker import (  # noqa: F401
    FrameIndexLookup,
    RepresentativeFrame,
    RepresentativePicker,
    TrajectoryFrameLocator,
    TrajectorySegment,
    build_frame_index_lookup,
)
from .uncertainty import UncertaintyQuantifier, UncertaintyResult  # noqa: F401
