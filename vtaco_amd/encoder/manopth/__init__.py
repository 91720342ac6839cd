"""What the reference keeps under src/encoder/manopth/ and this package mirrors: ``UpSampleLayer``."""
from .upsample_layer import UpSampleLayer  # noqa: F401
