"""Drop-in for the absent third-party package `dICP` (`from dICP.ICP import ICP`)."""
from mm_masking_amd.dICP.normals import estimate_normals, with_normals  # noqa: F401,E402
