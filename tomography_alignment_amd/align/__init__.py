"""Pre-alignment: `from tomography_alignment_amd.align import align_cc` mirrors the reference's `from align import align_cc`."""
