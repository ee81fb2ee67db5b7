"""fdeflate_amd -- MI355X-native batched DEFLATE codec behind fdeflate's PNG-path API.

Public surface mirrors image-rs/fdeflate (reference src/lib.rs:29-36) for the hot path:
decompress_to_vec, decompress_to_vec_bounded, compress_to_vec_ultra_fast, DecompressionError,
plus the batched device entry points.  See DESIGN.md / INTEGRATION.md.
"""
from .api import *  # noqa: F401,F403
from .api import __all__  # noqa: F401
