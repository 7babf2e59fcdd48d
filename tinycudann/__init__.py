"""Drop-in for the `tinycudann` package SplatLoc imports (models/encoding.py:3): the grid encodings of `tcnn.Encoding`,
MI355X-native (splatloc_amd/grid_encoding.py).  Networks and the non-grid encodings are not part of it."""
from splatloc_amd.grid_encoding import Encoding  # noqa: F401

__all__ = ["Encoding"]
