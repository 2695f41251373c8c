"""What goes with CarveEngine.hull_geodesic on the host: the default palette of paint_geodesic.  The pass itself is
vc_hull_geodesic."""
import numpy as np

from .clusters import PALETTE as _FIGURES

MAX_K = 32
# 33 colours, RGB: entry 0 (the region of the seed set) is grey, entry k paints the region of extremity k
PALETTE = np.vstack([np.array([(200, 200, 200)], dtype=np.uint8), np.tile(_FIGURES, (2, 1))])
UNREACHED_RGB = (255, 0, 255)
