"""Offline helpers of the reference: the two BAM down-samplers used for the
titration experiments, the theoretical limit-of-detection script, and `ds_allele_fraction`, the kit's third
down-sampler, which its README names and does not ship (semantics: DESIGN.md, "--dsAF").  Host-only Python; nothing here is on
the device path."""
