"""polytope_amd -- MI355X (gfx950) engine for the batched small-LP hot path of
tulip-control/polytope: Chebyshev-ball / redundancy / bounding-box LPs behind `reduce`,
`intersect`, `region_diff`; dense containment behind `contains`/`is_inside`; the
distance / furthest-point kernels of `quickhull`.

Drop-in surface: the package root carries the names the reference's root carries
(polytope/__init__.py:35-44) for everything on that path, so

    import polytope_amd as polytope
    polytope.solvers.default_solver = 'hip'

is the whole switch.  `grid_region` (and plotting) are outside the hot path
and are not provided.  `projection` and its helpers are reachable where the reference defines them,
as `polytope.polytope.projection` (and `Polytope.project`), not at the package root; on 'hip' its
Fourier-Motzkin steps run on the device.  The batched entry points (`*_batch`, no reference
counterpart, `projection_batch` among them) sit beside them.

The compute path is hand-written HIP (polytope_amd/csrc, built into libplp_hip.so and
reached through the C ABI of include/plp.h).  There is no CPU fallback: without the
library or without a gfx950 device the 'hip' backend raises.
"""
from . import _lib  # noqa: F401
from . import solvers  # noqa: F401
from .polytope import (  # noqa: F401
    Polytope, Region,
    is_empty, is_fulldim, is_convex, is_adjacent, is_subset,
    reduce, separate, box2poly,
    cheby_ball, bounding_box, envelope, extreme, qhull,
    is_inside, union, mldivide, intersect, intersect_pairs, volume, volume_exact, nearest, distance,
    distance_pairs, set_distance,
)
from .prop2partition import (  # noqa: F401
    Partition, MetricPartition, find_adjacent_regions, adjacency_sparse, overlap_sparse, overlay)
from . import polytope, prop2partition, quickhull  # noqa: F401,E402  (submodules, as `polytope.polytope` etc.)
from .batch import (  # noqa: F401
    lpsolve_batch, cheby_ball_batch, bbox_batch, reduce_batch, contains_batch, assign_batch, adjacent_pairs, keep_to_bool,
    verify_careful_lps, lp_histograms, projection_batch, volume_batch, support_batch, subset_batch, extreme_batch, hull_batch,
    volume_exact_batch, locate_batch, locate_grid, projection_hull_batch, nearest_batch,
    adjacent_pairs_sparse, overlap_pairs_sparse, overlap_cross_sparse, box_pairs, pair_verdicts,
    pair_stacks, intersect_cross_sparse,   # (the packed intersect_pairs is batch.intersect_pairs: the root name is the Polytope-level call)
    # (likewise distance_pairs: the packed call is batch.distance_pairs)
)
from .polytope import region_diff_batch  # noqa: F401,E402  (the Polytope-level call; the packed one is batch.region_diff_batch)
from .polytope import envelope_batch, is_convex_batch  # noqa: F401,E402  (the raw launch is batch.envelope_outer_batch)

__version__ = "0.1.0"
