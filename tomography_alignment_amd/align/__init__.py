"""Pre-alignment: `from tomography_alignment_amd.align import align_cc` mirrors the reference's `from align import align_cc`;
`consistency` (shifts from the projections' own moments) has no counterpart there."""
from . import consistency  # noqa: F401
from .consistency import Consistency, estimate_shifts, gauge_fix, marginals  # noqa: F401
