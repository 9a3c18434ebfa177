"""Stand-in for imgaug (not installed here): lav/utils/augmenter.py builds `augment(prob)` from imgaug.augmenters at dataset
construction; with this stand-in every augmenter is the identity, so a reference SegmentationDataset returns its images
unaugmented - what this repository's 'seg' loader does (tests/golden/make_golden_seg.py)."""
from . import augmenters  # noqa: F401
