"""Carves the reference's own scene (4 calibrated cameras + frame-0 MOG masks, committed fixtures) on the
GPU and writes the visual hull as a coloured point cloud (PLY) -- what the reference hands to its OpenGL
viewer after `G` is pressed.   python scripts/demo.py [grid=128] [out=hull.ply] [camera|visible|photo] [--render DIR]
[--smooth] [--textured] [--mesh PATH] [--normals] [--footprint centre|any|all] [--temporal T] [--frames F] [--noise P] [--close MM] [--open MM] [--clusters K] [--cluster-paint] [--extremities K] [--geodesic-paint labels|distance] [--measure [all|clusters|geodesic|components]] [--skeleton curve|point] [--skeleton-anchors extrema] [--shell [LEVEL]] [--save-hull PATH] [--subtract PATH] [--clip PATH] [--motion [BLOCK]] [--motion-paint] [--help] (`visible`: every surface voxel coloured by the cameras that see it, assignment.configure(color_mode="visible");
`photo`: the visual hull refined by photo-consistency carving and coloured that way, assignment.configure(hull="photo");
out `-`: no PLY; --render DIR: ray-cast images of the hull on the device, 8 orbit views at 1920x1080 and the 4 calibrated
cameras at mask size, as PNG when Pillow is importable, else binary PPM; --mesh PATH: the hull's surface mesh in world mm,
its vertices refined against the silhouettes on the device and coloured by the voxels, as binary PLY; --footprint: the carve's rule, assignment.configure(footprint=...) -- `any` keeps a
voxel when any pixel its whole cell projects to is foreground (the outer hull), `all` when all of them are (the inner hull);
--open MM: the hull opened by a ball of MM millimetres on the device after the carve, assignment.configure(hull_open_mm=MM) --
what is thinner than the ball leaves the hull; --close MM: the hull closed by a ball of MM millimetres on the device after the
carve and before any opening, assignment.configure(hull_close_mm=MM) -- tunnels and dents narrower than the ball are filled, which
is what a hole in one camera's mask carves; --smooth (with --render): every hit shaded by the hull's surface normal under a
headlight, assignment.render_views(smooth=True), instead of the six face brightnesses; --textured (with --render; colour mode `visible`, the default with it): every hit refined
along its ray against the silhouettes and coloured from the camera images that see it, assignment.render_views(textured=True); --lit (with --render, also with --smooth): cast shadows, ambient occlusion and a
chequered floor under a point light above the first camera, assignment.render_views(lit=True);
--normals (with --mesh): the PLY carries
nx, ny, nz per vertex, assignment.surface_mesh(normals=True); --clusters K: the hull split into K figures on the floor plane on
the device, assignment.configure(clusters=K) -- their floor positions in world mm and their sizes are printed; --cluster-paint
(with --clusters): every voxel in its figure's colour, in the PLY, the --render images and the --mesh;
--extremities K: geodesic distances through the hull from its floor contact and its K extremities by farthest-point selection on
the device, assignment.configure(extremities=K) -- their world positions and distances are printed; --geodesic-paint
labels|distance (with --extremities): every voxel in its region's colour or a grey ramp of its distance, in the PLY, the --render
images and the --mesh;
--measure [SOURCE]: the hull's figures measured on the device, assignment.configure(measure=SOURCE) -- one line per group with its
volume, boundary area, centroid, principal standard deviations, lean and height in world mm; SOURCE all (the default, the whole
hull), clusters (with --clusters K), geodesic (with --extremities K: the regions) or components (with the component filter);
--skeleton curve|point [--skeleton-anchors extrema]: the hull thinned to a one-voxel-wide skeleton with its topology on the
device, assignment.configure(skeleton=...) -- its voxels, end points, junctions and length in mm are printed; with
--skeleton-anchors extrema (and --extremities K) the floor contact and the extremities are pinned;
--shell [LEVEL]: only what an opaque cube viewer can show -- the voxels with an exposed face, listed on the device with the
viewer's arrays, assignment.configure(output="shell", output_level=LEVEL); survivors, shell, its share and the exposed faces are
printed and the PLY holds the shell; LEVEL 1..6 (default 0) lists the cells of a grid 2^LEVEL times coarser with averaged colours;
--temporal T [--frames F] [--noise P]: F frames (default 16) of the committed masks, each with a share P (default 0.02) of its
pixels flipped by a generator seeded with 7000 + the frame number, are carved one after the other and every hull is replaced by
the vote of the last T hulls on the device, assignment.configure(temporal_window=T) -- the voxels that change between consecutive
raw hulls and between consecutive voted hulls are printed per frame, and the last voted hull is what is written;
--temporal T --temporal-motion [BLOCK]: the motion-compensated vote, assignment.configure(temporal_window=T,
temporal_motion=(BLOCK, None, 4)) with BLOCK 4, 8 (the default) or 16, on a source that moves: frame t has its masks rolled by 2 t
columns, with the --noise flips on top -- per frame the raw, the aligned (what the block field does not explain) and the voted
change are printed with the listed and moved blocks (with it, --motion may stand beside --temporal: both want the rolled source);
--save-hull PATH: the hull as it stands after every pass (grid, bounds, records) as an .npz, CarveEngine.save_hull;
--subtract PATH / --clip PATH: a hull saved that way is subtracted from / intersected with every frame's hull on the device right
after the carve, assignment.configure(hull_subtract=PATH, hull_clip=PATH) -- the voxels each takes away are printed;
--motion [BLOCK] [--motion-paint] [--frames F]: F frames (default 4) of the committed masks, frame t rolled by 2 t columns, are
carved one after the other and from the second on the block motion against the previous frame's hull is estimated on the device,
assignment.configure(motion_block=BLOCK) with BLOCK 4, 8 (the default) or 16 -- per frame the listed, unique and moved blocks, the
change before and after compensation and the median vector in mm are printed; --motion-paint: every voxel coloured by its block's
vector (grey = at rest), in the PLY, the --render images and the --mesh; --motion-levels L (1..3): the coarse-to-fine field,
assignment.configure(motion_levels=L), which finds vectors beyond the search range -- the line of a frame then also says how many
vectors were borrowed from a neighbouring block's prediction and the field's reach;
--help: this text)."""
import os, sys
if "--help" in sys.argv or "-h" in sys.argv:
    print(__doc__)
    sys.exit(0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fixtures_util as fx
from voxcarve import assignment

smooth = "--smooth" in sys.argv
if smooth:
    sys.argv.remove("--smooth")
textured = "--textured" in sys.argv
if textured:
    sys.argv.remove("--textured")
lit = "--lit" in sys.argv
if lit:
    sys.argv.remove("--lit")
if lit and textured:
    sys.exit("--lit lights the voxel render; --textured takes its colours from the camera images")
with_normals = "--normals" in sys.argv
if with_normals:
    sys.argv.remove("--normals")
clusters = 0
if "--clusters" in sys.argv:
    k = sys.argv.index("--clusters")
    clusters = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
cluster_paint = "--cluster-paint" in sys.argv
if cluster_paint:
    sys.argv.remove("--cluster-paint")
extremities = 0
if "--extremities" in sys.argv:
    k = sys.argv.index("--extremities")
    extremities = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
geodesic_paint = None
if "--geodesic-paint" in sys.argv:
    k = sys.argv.index("--geodesic-paint")
    geodesic_paint = sys.argv[k + 1]
    del sys.argv[k:k + 2]
measure = None
if "--measure" in sys.argv:
    k = sys.argv.index("--measure")
    measure = "all"
    if k + 1 < len(sys.argv) and sys.argv[k + 1] in ("all", "clusters", "geodesic", "components"):
        measure = sys.argv[k + 1]
        del sys.argv[k + 1]
    del sys.argv[k]
skeleton = skeleton_anchors = None
if "--skeleton" in sys.argv:
    k = sys.argv.index("--skeleton")
    skeleton = sys.argv[k + 1]
    del sys.argv[k:k + 2]
if "--skeleton-anchors" in sys.argv:
    k = sys.argv.index("--skeleton-anchors")
    skeleton_anchors = sys.argv[k + 1]
    del sys.argv[k:k + 2]
shell_level = None
if "--shell" in sys.argv:
    k = sys.argv.index("--shell")
    shell_level = 0
    if k + 1 < len(sys.argv) and sys.argv[k + 1] in ("0", "1", "2", "3", "4", "5", "6"):
        shell_level = int(sys.argv[k + 1])
        del sys.argv[k + 1]
    del sys.argv[k]
render_dir = None
if "--render" in sys.argv:
    k = sys.argv.index("--render")
    render_dir = sys.argv[k + 1]
    del sys.argv[k:k + 2]
mesh_path = None
if "--mesh" in sys.argv:
    k = sys.argv.index("--mesh")
    mesh_path = sys.argv[k + 1]
    del sys.argv[k:k + 2]
footprint = "centre"
if "--footprint" in sys.argv:
    k = sys.argv.index("--footprint")
    footprint = sys.argv[k + 1]
    del sys.argv[k:k + 2]
open_mm = 0.0
if "--open" in sys.argv:
    k = sys.argv.index("--open")
    open_mm = float(sys.argv[k + 1])
    del sys.argv[k:k + 2]
close_mm = 0.0
if "--close" in sys.argv:
    k = sys.argv.index("--close")
    close_mm = float(sys.argv[k + 1])
    del sys.argv[k:k + 2]
save_hull = subtract = clip = None
for flag in ("--save-hull", "--subtract", "--clip"):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        value = sys.argv[k + 1]
        del sys.argv[k:k + 2]
        if flag == "--save-hull":
            save_hull = value
        elif flag == "--subtract":
            subtract = value
        else:
            clip = value
motion_block = 0
if "--motion" in sys.argv:
    k = sys.argv.index("--motion")
    motion_block = 8
    if k + 1 < len(sys.argv) and sys.argv[k + 1] in ("4", "8", "16"):
        motion_block = int(sys.argv[k + 1])
        del sys.argv[k + 1]
    del sys.argv[k]
motion_levels = 0
if "--motion-levels" in sys.argv:
    k = sys.argv.index("--motion-levels")
    if not motion_block or k + 1 >= len(sys.argv) or sys.argv[k + 1] not in ("0", "1", "2", "3"):
        sys.exit("--motion-levels L (0..3) is a setting of --motion")
    motion_levels = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
motion_paint = "--motion-paint" in sys.argv
if motion_paint:
    sys.argv.remove("--motion-paint")
temporal_motion = None
if "--temporal-motion" in sys.argv:
    k = sys.argv.index("--temporal-motion")
    temporal_motion = (8, None, 4)
    if k + 1 < len(sys.argv) and sys.argv[k + 1] in ("4", "8", "16"):
        temporal_motion = (int(sys.argv[k + 1]), None, 4)
        del sys.argv[k + 1]
    del sys.argv[k]
    if "--temporal" not in sys.argv:
        sys.exit("--temporal-motion is a setting of --temporal T")
if motion_block and "--temporal" in sys.argv and temporal_motion is None:
    sys.exit("--motion rolls the masks from frame to frame, --temporal flips their pixels: one of the two")
temporal, n_frames, noise = 0, 4 if motion_block else 16, 0.02
for flag, conv in (("--temporal", int), ("--frames", int), ("--noise", float)):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        value = conv(sys.argv[k + 1])
        del sys.argv[k:k + 2]
        if flag == "--temporal":
            temporal = value
        elif flag == "--frames":
            n_frames = value
        else:
            noise = value
g = int(sys.argv[1]) if len(sys.argv) > 1 else 128
out = sys.argv[2] if len(sys.argv) > 2 else "hull.ply"
color_mode = sys.argv[3] if len(sys.argv) > 3 else ("visible" if textured else "camera")
if textured and color_mode != "visible":
    sys.exit("--textured needs the colour mode `visible`: its depth maps say which cameras see a point")
hull = "photo" if color_mode == "photo" else "visual"
color_mode = "visible" if color_mode == "photo" else color_mode
masks = fx.golden_masks()
frames = [np.dstack([m // 2 + 60, m // 3 + 40, 255 - m // 2]).astype(np.uint8) for m in masks]   # any BGR image
sets = [(frames, masks)]
if temporal:
    sets = []
    for t in range(n_frames):
        rng = np.random.default_rng(7000 + t)
        moved = [np.roll(m, 2 * t, axis=1) for m in masks] if temporal_motion else masks
        sets.append((frames, [np.where(rng.random(m.shape) < noise, 255 - m, m).astype(np.uint8) for m in moved]))
if motion_block and not temporal:
    sets = [(frames, [np.roll(m, 2 * t, axis=1) for m in masks]) for t in range(n_frames)]
assignment.configure(frame_source=assignment.StaticFrameSource(sets), temporal_window=temporal, temporal_motion=temporal_motion, motion_block=motion_block,
                     motion_paint=motion_paint, motion_levels=motion_levels,
                     data_path=os.path.join(fx.GOLDEN, "data"), color_mode=color_mode, hull=hull, footprint=footprint,
                     hull_open_mm=open_mm, hull_close_mm=close_mm, clusters=clusters, cluster_paint=cluster_paint,
                     extremities=extremities, geodesic_paint=geodesic_paint if extremities else None,
                     min_component_voxels=1 if measure == "components" else 0, measure=measure,
                     skeleton=skeleton, skeleton_anchors=skeleton_anchors if skeleton else None,
                     output="all" if shell_level is None else "shell", output_level=shell_level or 0,
                     hull_subtract=subtract, hull_clip=clip)
pos, col = assignment.set_voxel_positions(g, g // 2, g)          # the reference's call: (width, height, depth)
if temporal:
    raw_sum = out_sum = 0
    for t in range(n_frames):
        if t:
            pos, col = assignment.set_voxel_positions(g, g // 2, g)
        ts = assignment.temporal()
        print("frame %2d: %d hulls, on %d off %d: raw hull %d voxels (%d changed), voted hull %d voxels (%d changed; %d restored, %d dropped), "
              "%.3f ms" % (t, ts["frames"], ts["on"], ts["off"], ts["survivors_before"], ts["raw_changed"], ts["survivors_after"],
                           ts["out_changed"], ts["added"], ts["removed"], ts["temporal_ms"]))
        if temporal_motion:
            print("          change against the last hull: raw %d, aligned %d, voted %d; %d of %d blocks listed, %d moved, %d at the range"
                  % (ts["raw_changed"], ts["aligned_changed"], ts["out_changed"], ts["listed"], ts["blocks"], ts["moved"], ts["clipped"]))
        if t >= temporal:
            raw_sum += ts["raw_changed"]
            out_sum += ts["out_changed"]
    print("flicker over frames %d..%d: %d voxels between raw hulls, %d between voted hulls" % (temporal, n_frames - 1, raw_sum, out_sum))
if motion_block and not temporal:                                # (beside --temporal the vote's lines above say what moved)
    for t in range(1, n_frames):
        pos, col = assignment.set_voxel_positions(g, g // 2, g)
        mo = assignment.motion()
        ms, med = mo["stats"], mo["description"]["median_mm"]
        print("frame %2d: %d of %d blocks listed, %d unique, %d moved, %d at the range; change %d -> %d voxels; median vector "
              "x %.1f y %.1f z %.1f mm (%.3f ms on the device)" % (t, ms["listed"], ms["blocks"], ms["unique"], ms["moved"], ms["clipped"],
                                                                   ms["cost0_sum"], ms["cost_sum"], med[0], med[1], med[2], ms["motion_ms"]))
        if motion_levels:
            print("          %d levels, vectors up to %d voxels: %d displacements tried, %d vectors borrowed from a neighbour's prediction"
                  % (ms["levels"], ms["reach"], ms["evaluated"], ms["borrowed"]))
if subtract or clip:
    for name, st in assignment.hull_ops().items():
        print("%s: %d of %d voxels leave the hull, %d stay (%d in the operand; %.3f ms on the device)" %
              (name, st["removed"], st["survivors_before"], st["survivors_after"], st["other"], st["setop_ms"]))
if save_hull:
    assignment._engine.save_hull(save_hull)
    print("hull of %d voxels -> %s" % (assignment._engine.count, save_hull))
rgb = (col * 255.0 + 0.5).astype(np.uint8)
if out != "-":
    with open(out, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(pos))
        for p, c in zip(pos, rgb):
            f.write("%g %g %g %d %d %d\n" % (p[0], p[1], p[2], c[0], c[1], c[2]))
print("%d voxels of the %dx%dx%d grid survive all 4 views (footprint %s, %sopened by %g mm) -> %s; extent x %.2f..%.2f, y %.2f..%.2f, z %.2f..%.2f" %
      (len(pos) if shell_level is None else assignment.shell()["survivors"], g, g, g, footprint, "closed by %g mm, " % close_mm if close_mm > 0 else "", open_mm, out, pos[:, 0].min(), pos[:, 0].max(), pos[:, 1].min(), pos[:, 1].max(), pos[:, 2].min(), pos[:, 2].max()))
if shell_level is not None:
    sh = assignment.shell()
    print("shell (level %d, cubes x%d on a %dx%dx%d grid): %d survivors in %d cells, %d with an exposed face (%.1f %% of the survivors); "
          "faces -x %d +x %d -y %d +y %d -z %d +z %d (%.3f ms on the device)" %
          ((sh["level"], sh["cube_scale"]) + tuple(sh["dims"]) + (sh["survivors"], sh["cells_on"], sh["shell"],
           100.0 * sh["shell"] / max(sh["survivors"], 1)) + tuple(sh["faces"]) + (sh["shell_ms"],)))
if clusters:
    cl = assignment.clusters()
    print("clusters: %d figures in %d rounds (%s, %.3f ms on the device)" % (clusters, cl["iterations"],
                                                                              "converged" if cl["converged"] else "not converged", cl["clusters_ms"]))
    for k in range(clusters):
        print("  figure %d: floor position x %.1f y %.1f mm, %d voxels in %d columns" % (k, cl["figures"]["centre_mm"][k, 0], cl["figures"]["centre_mm"][k, 1],
                                                                                 cl["figures"]["voxels"][k], cl["figures"]["columns"][k]))
if extremities:
    ge = assignment.extremities()
    print("extremities: %d found from %d floor voxels, %d of %d voxels reached, farthest %.1f mm (%d rounds, %.3f ms on the device)" %
          (ge["extremities"], ge["seeds"], ge["reached"], ge["survivors"], ge["max_d"] / 1000.0, ge["rounds"], ge["geodesic_ms"]))
    for k in range(ge["extremities"]):
        w = ge["extrema"]["world_mm"][k]
        print("  extremity %d: voxel %d at x %.1f y %.1f z %.1f mm, %.1f mm along the hull, path of %d voxels" %
              (k + 1, ge["extrema"]["voxel"][k], w[0], w[1], w[2], ge["extrema"]["d_mm"][k], len(ge["paths"][k])))
if measure:
    ms = assignment.measurements()
    w = ms["world"]
    print("measure: %d groups by %s, %d of %d voxels in a group (%.3f ms on the device; areas are the voxel boundary's)" %
          (ms["groups"], measure, ms["measured"], ms["survivors"], ms["measure_ms"]))
    for k in range(ms["groups"]):
        print("  group %d: %d voxels, volume %.4g mm3, area %.4g mm2, centroid x %.1f y %.1f z %.1f mm, std %.1f %.1f %.1f mm, lean %.1f deg, "
              "height %.1f mm" % ((k, w["voxels"][k], w["volume_mm3"][k], w["area_mm2"][k]) + tuple(w["centroid_mm"][k]) +
                                   tuple(w["std_mm"][k]) + (w["lean_deg"][k], w["height_mm"][k])))
if skeleton:
    sk = assignment.skeleton()
    print("skeleton (%s): %d voxels of %d, %d end points, %d junctions, %.1f mm of edges; %d passes, %d anchors (%.3f ms on the device)" %
          (skeleton, sk["stats"]["kept"], sk["stats"]["survivors"], sk["stats"]["endpoints"], sk["stats"]["junctions"],
           sk["description"]["length_mm"], sk["stats"]["passes"], sk["stats"]["anchors"], sk["stats"]["thin_ms"]))


def write_image(path, img):
    try:
        from PIL import Image
    except ImportError:
        with open(path + ".ppm", "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
            f.write(np.ascontiguousarray(img).tobytes())
        return path + ".ppm"
    Image.fromarray(img).save(path + ".png")
    return path + ".png"


if render_dir:
    from voxcarve import camera
    os.makedirs(render_dir, exist_ok=True)
    shade = (200, 200, 225, 225, 255, 150, 255)        # x sides, y sides, top (rays along +z: up is -z), bottom, inside
    orbit = camera.orbit(8, 4500.0, 25.0, 1500.0, 1080, 1920)
    if textured:
        r = assignment.render_views(orbit, 1920, 1080, textured=True)
        c = assignment.render_views(textured=True)
        ts = r["texture_stats"]
        print("textured: %d of %d hits refined along their rays, %d coloured from the camera images, %d kept the voxel colour "
              "(%.2f ms for 8 views on the device)" % (ts["refined"], ts["hits"], ts["textured"], ts["fallback"], ts["texture_ms"]))
    elif lit:
        r = assignment.render_views(orbit, 1920, 1080, lit=True, smooth=smooth)
        c = assignment.render_views(lit=True, smooth=smooth)
        ls = r["light_stats"]
        print("lit: %d hull and %d floor pixels, %d in shadow, %d turned from the light, %d secondary rays "
              "(%.2f ms for 8 views on the device)" % (ls["hull_pixels"], ls["floor_pixels"], ls["shadowed"], ls["facing_away"],
                                                        ls["rays_walked"], ls["light_ms"]))
    elif smooth:
        r = assignment.render_views(orbit, 1920, 1080, smooth=True)
        c = assignment.render_views(smooth=True)
    else:
        r = assignment.render_views(orbit, 1920, 1080, shade=shade)
        c = assignment.render_views(shade=shade)
    paths = [write_image(os.path.join(render_dir, "orbit_%d" % k), img) for k, img in enumerate(r["rgb"])]
    paths += [write_image(os.path.join(render_dir, "cam%d" % (k + 1)), img) for k, img in enumerate(c["rgb"])]
    print("%d images -> %s (orbit: %.2f ms for 8 views, %d of %d pixels hit)" % (len(paths), render_dir, r["stats"]["render_ms"],
                                                                              r["stats"]["hits"], r["stats"]["pixels"]))

if mesh_path:
    from voxcarve.voxel_reconstruction import write_ply
    m = assignment.surface_mesh(8, normals=with_normals)
    write_ply(mesh_path, m["verts"], m["faces"], m["rgb"], normals=m.get("normals"))
    st = m["stats"]
    print("mesh: %d vertices (%d refined), %d faces -> %s (%.2f ms on the device)" % (st["n_verts"], st["refined"], st["n_faces"],
                                                                                  mesh_path, st["surface_ms"]))
