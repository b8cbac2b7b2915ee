from .alignment_pixels import AlignmentPixels, align_pixels_shift  # noqa: F401
from .alignment_spice_pixel import AlignmentSpicePixel  # noqa: F401
from .pixel_alignment_results import PixelAlignmentResults  # noqa: F401
from .local_shift_field import LocalShiftField  # noqa: F401
