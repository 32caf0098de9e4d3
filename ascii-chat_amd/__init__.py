"""ascii-chat_amd: Python-side plumbing for libasciichat_hip.so (the MI355X-native render path).

The product is the C-ABI shared library built from csrc/ (see include/asciichat_hip.h and
include/asciichat_render.h); this package only loads it through ctypes for the test-suite and bench.py
and uses torch for device memory, streams and torch.distributed.  There is no Python or CPU
implementation of the render path here: if the library or a GPU is missing, calls fail loudly.

The directory name contains a hyphen, so import it with the helper in __graft_entry__.py:
    from __graft_entry__ import load_package; achip = load_package()
"""
from .binding import *  # noqa: F401,F403
from . import distributed  # noqa: F401
from .raster import *  # noqa: F401,F403  (libasciichat_raster.so: loaded at the first Raster, not here)
from .yuv import *  # noqa: F401,F403  (libasciichat_yuv.so: loaded at the first Yuv or yuv_convert, not here)
from .yuvgrid import *  # noqa: F401,F403  (libasciichat_yuvgrid.so: loaded at the first YuvGrid, not here)
from .yuvbox import *  # noqa: F401,F403  (libasciichat_yuvbox.so: loaded at the first YuvBox or yuvbox_downscale, not here)
from .yuvboxgrid import *  # noqa: F401,F403  (libasciichat_yuvboxgrid.so: loaded at the first YuvBoxGrid, not here)
from .pix import *  # noqa: F401,F403  (libasciichat_pix.so: loaded at the first Pix, pix_convert or pix_downscale, not here)
from .pixgrid import *  # noqa: F401,F403  (libasciichat_pixgrid.so: loaded at the first PixGrid, not here)
