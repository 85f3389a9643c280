"""Drop-in for the ``dICP`` package (lisusdaniil/dICP, absent upstream): ``from dICP.ICP import ICP``."""
from .ICP import ICP  # noqa: F401
from .normals import estimate_normals, with_normals  # noqa: F401
from .voxel import voxel_downsample  # noqa: F401
