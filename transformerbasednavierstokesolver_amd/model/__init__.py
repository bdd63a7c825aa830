"""Model modules mirroring the reference's `model/` package (structured-mesh-2D, structured-mesh-3D, irregular-mesh and
structured-mesh-2D auto-encoder families)."""
from . import Transolver_Structured_Mesh_2D, Transolver_Irregular_Mesh, SOL_Transolver_Structured_Mesh_2D, Physics_Attention  # noqa: F401
from . import Transolver_Structured_Mesh_3D  # noqa: F401
from . import Transolver_Structured_Mesh2D_Encoder  # noqa: F401
