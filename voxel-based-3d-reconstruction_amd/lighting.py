"""The lit pass's side of the C ABI (vc_light_render, include/voxcarve.h) and its defaults: the light and the stats as the
library lays them out, a light above a camera, a floor under the grid.  CarveEngine.light_render / render_lit make the calls."""
import ctypes

import numpy as np

AUTO_FLOOR_CELL_MM = 250.0
AUTO_FLOOR_RGB = ((96, 96, 96), (160, 160, 160))
DEFAULT_LIGHT_LIFT_MM = 1000.0


class Light(ctypes.Structure):               # vc_light_t
    _fields_ = [("pos", ctypes.c_double * 4), ("ambient", ctypes.c_uint32), ("smooth", ctypes.c_uint32), ("ao_reach", ctypes.c_double),
                ("floor", ctypes.c_uint32), ("floor_z", ctypes.c_double), ("floor_rect", ctypes.c_double * 4),
                ("floor_cell_mm", ctypes.c_double), ("floor_rgb", (ctypes.c_uint8 * 3) * 2)]


class LightStats(ctypes.Structure):          # vc_light_stats_t
    _fields_ = [("pixels", ctypes.c_uint64), ("hull_pixels", ctypes.c_uint64), ("floor_pixels", ctypes.c_uint64),
                ("shadowed", ctypes.c_uint64), ("facing_away", ctypes.c_uint64), ("rays_walked", ctypes.c_uint64),
                ("cells_visited", ctypes.c_uint64), ("blocks_skipped", ctypes.c_uint64), ("light_ms", ctypes.c_float)]


def auto_floor(grid, bounds):
    """The floor of floor="auto": z = the grid's largest z boundary (world up is -z: the plane the lowest voxels stand on), the
    rectangle = the x and y bounds grown by half their span on each side, cells of 250 mm in two greys."""
    nz = int(grid[2])
    sz = (float(bounds[5]) - float(bounds[4])) / float(nz - 1)
    z = (float(bounds[4]) - 0.5 * sz) + float(nz) * sz
    gx, gy = 0.5 * (float(bounds[1]) - float(bounds[0])), 0.5 * (float(bounds[3]) - float(bounds[2]))
    return {"z": z, "rect": (float(bounds[0]) - gx, float(bounds[1]) + gx, float(bounds[2]) - gy, float(bounds[3]) + gy),
            "cell_mm": AUTO_FLOOR_CELL_MM, "rgb": AUTO_FLOOR_RGB}


def light_above(view):
    """(x, y, z, 1): a point light 1000 mm above (towards -z of) the centre -R^T t of a camera.Camera."""
    R = np.asarray(view.R, dtype=np.float64).reshape(3, 3)
    c = -(R.T @ np.asarray(view.tvec, dtype=np.float64).reshape(3))
    return (float(c[0]), float(c[1]), float(c[2]) - DEFAULT_LIGHT_LIFT_MM, 1.0)


def light_struct(light, ambient, smooth, ao_reach, floor, grid=None, bounds=None):
    """The vc_light_t of CarveEngine.light_render's arguments.  light: (x, y, z, w), or (x, y, z) for a point; floor: None, "auto"
    (needs grid and bounds) or a dict with z, rect (x0, x1, y0, y1), cell_mm and rgb (two RGB triples)."""
    pos = [float(v) for v in np.asarray(light, dtype=np.float64).reshape(-1)]
    if len(pos) == 3:
        pos.append(1.0)
    if len(pos) != 4:
        raise ValueError("light_render: light %r, expected (x, y, z, w) or (x, y, z)" % (light,))
    if not 0 <= int(ambient) <= 255:
        raise ValueError("light_render: ambient %r not in 0..255" % (ambient,))
    L = Light()
    L.pos[:] = pos
    L.ambient, L.smooth, L.ao_reach = int(ambient), 1 if smooth else 0, float(ao_reach)
    L.floor_cell_mm = 1.0
    if floor is not None:
        if isinstance(floor, str):
            if floor != "auto":
                raise ValueError('light_render: floor %r, expected None, "auto" or a dict' % (floor,))
            if grid is None:
                raise ValueError('light_render: floor="auto" needs a grid')
            floor = auto_floor(grid, bounds)
        missing = [k for k in ("z", "rect", "cell_mm", "rgb") if k not in floor]
        if missing:
            raise ValueError("light_render: the floor lacks %s" % ", ".join(missing))
        L.floor, L.floor_z, L.floor_cell_mm = 1, float(floor["z"]), float(floor["cell_mm"])
        L.floor_rect[:] = [float(v) for v in np.asarray(floor["rect"], dtype=np.float64).reshape(4)]
        rgb = np.asarray(floor["rgb"], dtype=np.uint8).reshape(2, 3)
        for k in range(2):
            L.floor_rgb[k][:] = [int(v) for v in rgb[k]]
    return L
