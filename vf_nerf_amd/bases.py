"""``get_dominant_bases`` with the reference's signature and return (utils/utils.py:216-233): the dominant directions of a mesh file as
a NumPy array, computed on the device by ``meshops.dominant_bases``.  ``dropin.install(patch_dominant_bases=True)`` puts it behind
``utils.utils.get_dominant_bases``.

Not a recording of the reference's numbers: the reference decimates with trimesh's edge collapse and clusters with scikit-learn's
default seeding (greedy k-means++ from NumPy's global random state); here the decimation is a vertex clustering chosen by bisection
(``meshops.simplify_to_faces``, AS SPECIFIED BY US) and the seeding is the deterministic farthest-point rule of ``cluster.kmeans``.  What
agrees with scikit-learn is the Lloyd iteration from given seeds.  The bases come in descending order of their counts; the reference's
order is whatever scikit-learn's seeding made it.
"""
from __future__ import annotations

import numpy as np

from . import meshops, ply


def get_dominant_bases(num_bases: int, decimation: float, path_to_bases: str) -> np.ndarray:
    """The mesh at ``path_to_bases`` (a PLY file, read by ``ply.read_ply``) decimated to ``decimation`` times its faces, the k-means
    centres of its vertex normals -> float64 [num_bases,3] on the host.  No CPU fallback: ``lib.VfnError`` without a device."""
    vertices, faces, _ = ply.read_ply(path_to_bases)
    return meshops.dominant_bases((vertices, faces), num_bases, decimation=decimation).bases.cpu().numpy()
