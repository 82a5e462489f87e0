// render_mhd.cpp -- the reference application's start-up sequence (main.cpp / gui/mainwindow.cpp:22-62, 229-238)
// without the GUI: load a MetaImage volume, the GUI-default (or a saved .tf) transfer function, one area light, an
// optional .hdr environment map; render N progressive frames (or, with -noise T, until the predicted RMSE of the tone-mapped
// image is <= T, at most N frames; with -adaptive T, 16 x 16 tiles stop once their predicted RMSE is <= T); write the image as TGA.
// -mip / -mean / -iso LEVEL draw one projection image instead (svr_render_projection): maximum intensity, mean intensity through the
// grey window -window LO HI (default 0 1), or the head-light shaded isosurface at LEVEL; -tfcolor colours them with the transfer function.
// -slice x|y|z POS draws the plane perpendicular to that axis at POS in [0, 1] across the volume (svr_render_slice; -window and -tfcolor
// apply); -slab THICKNESS mip|minip|mean thickens it into a slab (world units, one sample per pixel size); -stack N writes N parallel
// slices from POS to the far face as name_0000.tga ... in one launch (svr_render_slice_stack).
// -pick X Y (repeatable) renders no frame: it prints, one line per pick, where the ray of that pixel meets what the picture shows
// (svr_pick) -- -hit opacity A: the ray caster's opacity exceeds A (default, 0.5); -hit iso L: the isosurface at L; -hit max: the sample
// of the MIP value.
// -grow X Y LO HI picks at pixel (X, Y) with the -hit mode in force, grows the connected region of the voxels with raw value LO .. HI
// (0 .. 65535) around the picked voxel (svr_region_grow; -conn 6|18|26, default 6), prints its voxel count, volume, mean +- standard
// deviation, bounding box and surface area, and renders the volume with everything else removed (-keep, the default) or with the
// region removed (-remove) into the output image.  After -grow, -detach R, -fillholes, -open R, -close R, -dilate R and -erode R clean the
// region up, in command-line order (Canvas::DetachRegion, FillRegionHoles, MorphRegion; R = 1 .. 32 applications of the unit element
// -element 6|18|26, default 6): -detach cuts off what hangs on the picked structure by connections thinner than the element,
// -fillholes adds what the region encloses.  The measurements are printed once more after the last step, and that region is shown.
// -overlay FILL EDGE (opacities 0 .. 255) lays the region over the picture the run writes -- a slice, a stack, the ray caster's image, a MIP
// or an isosurface -- instead of cutting it out of the volume: the inside tinted with FILL, the outline with EDGE (svr_overlay_slice;
// svr_render_hits + svr_hit_ids + svr_overlay_ids for the 3D pictures).  -overlay-parts CONN labels the region first, so every
// connected part gets its own colour (Canvas::LabelRegion).
// -threshold LO HI is the alternative to -grow: the region is every voxel with raw value LO .. HI, with no pick (Canvas::ThresholdRegion);
// the line it prints gives the number of connected parts (-conn) next to the measurements.  -largest K keeps the K largest parts and
// -minsize N those of at least N voxels (Canvas::KeepLargestRegion, RemoveSmallRegions; connectivity -conn): clean-up steps taken in
// command-line order with the others, each printing the parts it found and kept and the measurements of what is left.  -detach starts
// from the picked voxel and is therefore not available after -threshold.
// -otsu CLASSES CLASS [SHIFT] stands where -threshold LO HI may stand: the window is class CLASS = 1 .. CLASSES (dark to bright) of the exact
// Otsu thresholds of the histogram of raw value >> SHIFT (Canvas::OtsuRegion; CLASSES = 2, or 3 with SHIFT >= 8; SHIFT is 8 by default).
// It prints the thresholds as raw values and the window, then goes on as -threshold with that window.  -auto-window PLO PHI sets the grey
// window of -slice / -mip / -mean to the quantiles PLO and PHI, in per mille, of the (filtered) voxels (Canvas::AutoWindow).  After -grow,
// -threshold or -otsu the median raw value of the region is printed with the measurements (Canvas::RegionMedian).
// -ball-dilate L, -ball-erode L, -ball-open L and -ball-close L are clean-up steps too, by a true ball of radius L > 0 in the units of the
// volume's spacing (Canvas::BallMorphRegion: the exact Euclidean distance map, any radius at the same cost); each prints the measurements
// of what is left.  -thickness prints, after the last step, the largest ball inscribed in the region and its centre voxel.
// -split L is the step that separates objects which touch: necks thinner than a ball of radius L > 0 are cut (Canvas::SplitRegion: erode
// by the ball, label the cores under -conn, give every voxel to the core nearest inside the region, take a cut of one voxel between the
// parts); it prints the number of parts, and -largest / -minsize after it choose among them.
// -median E N and -smooth SIGMA filter the voxels BEFORE they are segmented, in command-line order (Canvas::MedianVolume: the median over
// the unit element E = 6|18|26, N = 1 .. 64 times; Canvas::SmoothVolume: binomial smoothing of SIGMA > 0 in the units of the volume's
// spacing): -grow and -threshold then work on the filtered copy, and so does what they show.  -show-filtered draws the filtered copy
// in place of the loaded volume.
// -mesh FILE.stl|.ply writes the closed surface of the region that is left after all clean-up and selection steps (Canvas::
// ExtractRegionSurface, SaveSurface: surface nets in world coordinates; -relax N smooths it by N = 0 .. 64 constrained relaxation
// steps); -mesh-iso RAW FILE.stl|.ply writes the isosurface {raw value >= RAW} of the (filtered) voxels, with or without a region.  Each
// prints "mesh: V vertices, T triangles, volume ... mm^3, area ... mm^2", the region's line first.
// -seed X Y CLASS [RADIUS] (repeatable) and -growcut [GAIN SHIFT] are grow-from-seeds (Canvas::AddSeed, GrowFromSeeds: svr_region_growcut):
// every -seed picks at pixel (X, Y) like -grow and paints a stroke of class CLASS = 1, 2, ... -- the ball of RADIUS in the units of the
// spacing, twice the smallest spacing by default -- and -growcut gives every voxel of the region made by -grow / -threshold, or without
// one of the whole volume, to the class whose strokes reach it over the path that crosses the least contrast (a move costs 1 + GAIN *
// (|difference of the raw values| >> SHIFT), 1 and 0 by default).  -overlay then tints every class in its own colour and -save-parts
// writes the class map; -keep-class C makes class C the region, for the clean-up steps, -keep / -remove, -mesh and -save-mask.
// -crop X0 Y0 Z0 X1 Y1 Z1 (an inclusive voxel box, cut to the volume) and -resample MM [nearest|linear|area|auto] (the same spacing MM on
// every axis, in the units of the file's spacing; auto = linear where the grid gets finer, area where it gets coarser) change the grid
// right after the load, in command-line order (Canvas::CropVolume, ResampleVolume): everything after works on the new grid, drawn where
// it lay in the loaded volume.  -save-volume F writes the (filtered) voxels, -save-mask F the final region as u8 0 / 1, -save-parts F
// its connected parts (-conn) as a u32 label map, and -save-crop VOL MASK MARGIN the region's bounding box grown by MARGIN voxels, voxels
// and mask, as MetaImage files (.mhd + .raw, or .mha).  Each prints one line with the dimensions, the spacing and the time.
// -compare-mask F compares the final region with the mask in F (one byte per voxel, non-zero = set, the volume's dimensions: what
// -save-mask wrote, or a ground truth) and prints one line: Dice, Jaccard, the Hausdorff distance, its 95 % form and the average
// symmetric surface distance in the units of the spacing (Canvas::CompareRegionWithFile).
// -scissor inside|outside X0 Y0 X1 Y1 [X2 Y2 ...] cuts the region with a closed line drawn on the picture that is rendered, through its
// camera: two points are the corners of an inclusive pixel rectangle, three or more the vertices of a polygon in pixels; `inside` removes
// the voxels seen inside it, `outside` those seen outside (Canvas::ScissorRegion).  -scissor-slice x|y|z POS inside|outside|fill T X0 Y0 ...
// does the same on the slice picture of that axis and position, within the slab of thickness T around the plane (T = 0: the whole
// depth); `fill` adds the voxels instead (Canvas::ScissorRegionOnSlice, PaintRegionOnSlice).  Both come after the clean-up steps, in
// command-line order, and print the region they leave.
// -fill-between x|y|z fills the slices of that axis between the slices that hold a voxel of the region, by shape-based interpolation
// (Canvas::FillRegionBetweenSlices): what was drawn on every few slices with -scissor-slice ... fill, or thresholded in a volume that has
// only every few slices, becomes solid.  It comes after the scissors -- so after the clean-up steps, -largest among them -- and before
// -thickness, -mesh, -save-mask and the other outputs, and prints the keys, gaps and filled slices and the voxels before and after.
// -smooth-region median|gauss SIZE [N] smooths the ragged boundary of the region N times (1 by default) without shifting it
// (Canvas::SmoothRegion): `median` sets a voxel iff more than half of the window of edge SIZE around it is set, `gauss` keeps the upper
// half of the region smoothed binomially with sigma SIZE; SIZE is in the units of the spacing.  It comes after -fill-between and before
// the outputs.  -smooth-parts SIZE [N] smooths all parts at once by the mode of the window (Canvas::SmoothRegionParts): the classes of
// -growcut, before -keep-class picks one, or after the clean-up steps (-split among them) the parts of the region under -conn; parts
// stay disjoint and leave no gaps, and -save-parts and -overlay then get the smoothed parts unless a later step replaces the region.
// -density SIZE draws the local volume fraction of the region in the window of edge SIZE in place of the masked volume
// (Canvas::ShowRegionDensity).
//
//   render_mhd <volume.mhd> [-tf file.tf] [-env map.hdr] [-frames N] [-depth D] [-size W H] [-raycast] [-mip | -mean | -iso LEVEL] [-slice x|y|z POS] [-slab THICKNESS mip|minip|mean] [-stack N] [-window LO HI] [-tfcolor] [-pick X Y [-hit opacity A | iso L | max]] [-crop X0 Y0 Z0 X1 Y1 Z1 | -resample MM [nearest|linear|area|auto]]... [-median E N | -smooth SIGMA]... [-show-filtered] [-save-volume F] [-seed X Y CLASS [RADIUS]]... [-growcut [GAIN SHIFT]] [-keep-class C] [-auto-window PLO PHI] [-grow X Y LO HI | -threshold LO HI | -otsu CLASSES CLASS [SHIFT] [-conn 6|18|26] [-detach R | -fillholes | -open R | -close R | -dilate R | -erode R | -largest K | -minsize N | -ball-dilate L | -ball-erode L | -ball-open L | -ball-close L | -split L]... [-element 6|18|26] [-thickness] [-keep | -remove] [-overlay FILL EDGE [-overlay-parts CONN]] [-mesh FILE.stl|.ply [-relax N]] [-save-mask F] [-save-parts F] [-scissor inside|outside X0 Y0 X1 Y1 [X2 Y2 ...]]... [-scissor-slice x|y|z POS inside|outside|fill T X0 Y0 X1 Y1 [X2 Y2 ...]]... [-fill-between x|y|z] [-smooth-region median|gauss SIZE [N]] [-smooth-parts SIZE [N]] [-density SIZE] [-save-crop VOL MASK MARGIN] [-compare-mask F]] [-mesh-iso RAW FILE.stl|.ply] [-denoise-preview N] [-noise T] [-adaptive T] [-o out.tga]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>

#include "sunvolumerender/canvas.hpp"

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s volume.mhd [-tf f.tf] [-env m.hdr] [-frames N] [-depth D] [-size W H] [-raycast] [-mip | -mean | -iso LEVEL] [-slice x|y|z POS] [-slab THICKNESS mip|minip|mean] [-stack N] [-window LO HI] [-tfcolor] [-pick X Y [-hit opacity A | iso L | max]] [-crop X0 Y0 Z0 X1 Y1 Z1 | -resample MM [nearest|linear|area|auto]]... [-median E N | -smooth SIGMA]... [-show-filtered] [-save-volume F] [-seed X Y CLASS [RADIUS]]... [-growcut [GAIN SHIFT]] [-keep-class C] [-auto-window PLO PHI] [-grow X Y LO HI | -threshold LO HI | -otsu CLASSES CLASS [SHIFT] [-conn 6|18|26] [-detach R | -fillholes | -open R | -close R | -dilate R | -erode R | -largest K | -minsize N | -ball-dilate L | -ball-erode L | -ball-open L | -ball-close L | -split L]... [-element 6|18|26] [-thickness] [-keep | -remove] [-overlay FILL EDGE [-overlay-parts CONN]] [-mesh FILE.stl|.ply [-relax N]] [-save-mask F] [-save-parts F] [-scissor inside|outside X0 Y0 X1 Y1 [X2 Y2 ...]]... [-scissor-slice x|y|z POS inside|outside|fill T X0 Y0 X1 Y1 [X2 Y2 ...]]... [-fill-between x|y|z] [-smooth-region median|gauss SIZE [N]] [-smooth-parts SIZE [N]] [-density SIZE] [-save-crop VOL MASK MARGIN] [-compare-mask F]] [-mesh-iso RAW FILE.stl|.ply] [-denoise-preview N] [-noise T] [-adaptive T] [-o out.tga]\n", argv[0]); return 2; }
    std::string volume = argv[1], tfFile, envFile, out = "frame.tga";
    int frames = 16, depth = 1, W = 640, H = 640;                  // common.h:8-9
    int denoisePreview = 0;
    float noiseTarget = 0.f;                                        // 0: render exactly -frames frames
    float adaptiveTarget = 0.f;                                     // > 0: adaptive sampling, tiles stop at this predicted RMSE
    bool raycast = false, project = false;
    svr_projection_params proj = {SVR_PROJ_MIP, 0u, 0.5f, 0.f, 1.f};
    int sliceAxis = -1, stack = 0, slabMode = 0;                    // -slice: axis 0 / 1 / 2; -stack: slices; -slab: SVR_SLAB_*
    float slicePos = 0.5f, slabThickness = 0.f;
    std::vector<uint32_t> picks;                                    // -pick: (x, y) pairs
    svr_hit_params hitParams = {SVR_HIT_OPACITY, 0.5f, 0.5f};
    struct SeedStroke { int x, y, cls; double radius; };            // -seed X Y CLASS [RADIUS]: radius < 0 = twice the smallest spacing
    std::vector<SeedStroke> seeds;
    bool growcut = false;                                           // -growcut [GAIN SHIFT]: grow the strokes' classes; -keep-class C: one of them becomes the region
    int growGain = 1, growShift = 0, keepClass = 0;                 // (the gain and shift of svr_region_growcut_params_default)
    bool grow = false;                                              // -grow: pixel, raw window, connectivity, what to show
    int growX = 0, growY = 0, growLo = 0, growHi = 65535, growConn = 6, growMode = SVR_REGION_KEEP;
    bool threshold = false;                                         // -threshold: the whole window growLo .. growHi, no pick
    int otsuClasses = 0, otsuClass = 0, otsuShift = 8;              // -otsu CLASSES CLASS [SHIFT]: -threshold with the window of an Otsu class
    int autoLo = -1, autoHi = -1;                                   // -auto-window PLO PHI: the grey window from two quantiles, per mille
    bool overlay = false;                                           // -overlay FILL EDGE: tint the picture by the region, which is not cut out of the volume
    int overlayFill = 96, overlayEdge = 255, overlayParts = 0;      // -overlay-parts CONN: label the region first, one colour per part
    struct CleanStep { const char* name; int op; uint32_t radius; double length; };   // op: SVR_MORPH_*, 0 = -fillholes, -1 = -detach, -3 = -largest, -4 = -minsize (radius: K or N), -5 = -split (length: L), -10 - SVR_MORPH_* = -ball-* (length: L)
    std::vector<CleanStep> cleanSteps;                              // -detach / -fillholes / -open / -close / -dilate / -erode / -largest / -minsize / -ball-* / -split, in order
    int cleanElement = 6;
    bool thickness = false;                                         // -thickness: the largest inscribed ball of the final region
    struct FilterStep { int element; uint32_t iterations; double sigma; };     // -median E N (element != 0) or -smooth SIGMA
    std::vector<FilterStep> filterSteps;                            // in command-line order
    bool showFiltered = false;                                      // -show-filtered
    std::string meshFile, meshIsoFile;                              // -mesh FILE: the surface of the final region; -mesh-iso RAW FILE: the raw isosurface
    int meshRelax = -1, meshIsoLevel = 0;                           // -relax N (with -mesh): 0 .. SVR_MESH_MAX_RELAX relaxation steps
    struct GridStep { bool crop; int32_t lo[3], hi[3]; double mm; int mode; };   // -crop X0 Y0 Z0 X1 Y1 Z1 or -resample MM [mode]
    std::vector<GridStep> gridSteps;                                // applied right after the load, in command-line order
    std::string compareMaskFile;                                    // -compare-mask F: the final region against the mask in F
    struct ScissorStep { int axis; float pos; int op; float thickness; std::vector<double> polygon; };   // -scissor (axis -1) / -scissor-slice, in order
    std::vector<ScissorStep> scissorSteps;
    int fillBetweenAxis = -1;                                       // -fill-between x|y|z
    int smoothRegionOp = 0, smoothRegionN = 1, smoothPartsN = 1;    // -smooth-region median|gauss SIZE [N]; -smooth-parts SIZE [N]; -density SIZE
    double smoothRegionSize = 0.0, smoothPartsSize = -1.0, densitySize = -1.0;
    bool partsSmoothed = false;                                     // the canvas's label map is what -smooth-parts left
    const auto sizeArg = [](const char* a, double* v) {             // a length >= 0
        char* end = nullptr;
        *v = strtod(a, &end);
        return end != a && *end == '\0' && *v >= 0.0 && std::isfinite(*v);
    };
    const auto timesArg = [&](int* i, int* n) {                     // the optional [N] after a size: 1 .. 16
        if (*i + 1 >= argc || argv[*i + 1][0] == '-') return true;
        char* end = nullptr;
        const long v = strtol(argv[*i + 1], &end, 10);
        if (*end != '\0') return true;                              // (not a number: the next argument is something else)
        if (v < 1 || v > SVR_REGION_SMOOTH_MAX_ITERATIONS) return false;
        *n = (int)v;
        ++*i;
        return true;
    };
    std::string saveVolumeFile, saveMaskFile, savePartsFile, saveCropVolume, saveCropMask;   // -save-volume / -save-mask / -save-parts F, -save-crop VOL MASK MARGIN
    int saveCropMargin = 0;
    const auto meshName = [](const char* f) {                       // an export writes .stl or .ply
        const size_t n = strlen(f);
        return n > 4 && (!strcmp(f + n - 4, ".stl") || !strcmp(f + n - 4, ".ply"));
    };
    for (int i = 2; i < argc; ++i) {
        int cleanOp = -2;
        if (!strcmp(argv[i], "-detach")) cleanOp = -1;
        else if (!strcmp(argv[i], "-open")) cleanOp = SVR_MORPH_OPEN;
        else if (!strcmp(argv[i], "-close")) cleanOp = SVR_MORPH_CLOSE;
        else if (!strcmp(argv[i], "-dilate")) cleanOp = SVR_MORPH_DILATE;
        else if (!strcmp(argv[i], "-erode")) cleanOp = SVR_MORPH_ERODE;
        if (cleanOp != -2) {
            char* end = nullptr;
            const long r = i + 1 < argc ? strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || r < 1 || r > SVR_MORPH_MAX_RADIUS) {
                fprintf(stderr, "%s needs a radius R in 1 .. %d (got %s)\n", argv[i], SVR_MORPH_MAX_RADIUS, i + 1 < argc ? argv[i + 1] : "nothing");
                return 2;
            }
            cleanSteps.push_back(CleanStep{argv[i], cleanOp, (uint32_t)r, 0.0});
            ++i;
        }
        else if (!strcmp(argv[i], "-largest") || !strcmp(argv[i], "-minsize")) {
            const bool largest = argv[i][1] == 'l';
            char* end = nullptr;
            const long long v = i + 1 < argc ? strtoll(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || v < 1 || v > 0x7fffffffLL) {
                fprintf(stderr, "%s needs a %s >= 1 (got %s)\n", argv[i], largest ? "number of parts K" : "voxel count N", i + 1 < argc ? argv[i + 1] : "nothing");
                return 2;
            }
            cleanSteps.push_back(CleanStep{argv[i], largest ? -3 : -4, (uint32_t)v, 0.0});
            ++i;
        }
        else if (!strncmp(argv[i], "-ball-", 6)) {
            const char* what = argv[i] + 6;
            const int op = !strcmp(what, "dilate") ? SVR_MORPH_DILATE : !strcmp(what, "erode") ? SVR_MORPH_ERODE : !strcmp(what, "open") ? SVR_MORPH_OPEN
                         : !strcmp(what, "close") ? SVR_MORPH_CLOSE : 0;
            if (!op) { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
            char* end = nullptr;
            const double len = i + 1 < argc ? strtod(argv[i + 1], &end) : 0.0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(len > 0.0) || !std::isfinite(len)) {
                fprintf(stderr, "%s needs a radius L > 0 in the units of the spacing (got %s)\n", argv[i], i + 1 < argc ? argv[i + 1] : "nothing");
                return 2;
            }
            cleanSteps.push_back(CleanStep{argv[i], -10 - op, 0u, len});
            ++i;
        }
        else if (!strcmp(argv[i], "-split")) {
            char* end = nullptr;
            const double len = i + 1 < argc ? strtod(argv[i + 1], &end) : 0.0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(len > 0.0) || !std::isfinite(len)) {
                fprintf(stderr, "-split needs a neck radius L > 0 in the units of the spacing (got %s)\n", i + 1 < argc ? argv[i + 1] : "nothing");
                return 2;
            }
            cleanSteps.push_back(CleanStep{argv[i], -5, 0u, len});
            ++i;
        }
        else if (!strcmp(argv[i], "-median")) {
            char *e0 = nullptr, *e1 = nullptr;
            const long e = i + 2 < argc ? strtol(argv[i + 1], &e0, 10) : 0, n = i + 2 < argc ? strtol(argv[i + 2], &e1, 10) : 0;
            if (i + 2 >= argc || e0 == argv[i + 1] || *e0 != '\0' || e1 == argv[i + 2] || *e1 != '\0' || (e != 6 && e != 18 && e != 26) || n < 1 || n > SVR_FILTER_MAX_ITERATIONS) {
                fprintf(stderr, "-median needs an element E of 6, 18 or 26 and a number of passes N in 1 .. %d (got %s %s)\n", SVR_FILTER_MAX_ITERATIONS,
                        i + 1 < argc ? argv[i + 1] : "nothing", i + 2 < argc ? argv[i + 2] : "nothing");
                return 2;
            }
            filterSteps.push_back(FilterStep{(int)e, (uint32_t)n, 0.0});
            i += 2;
        }
        else if (!strcmp(argv[i], "-smooth")) {
            char* end = nullptr;
            const double sigma = i + 1 < argc ? strtod(argv[i + 1], &end) : 0.0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(sigma > 0.0) || !std::isfinite(sigma)) {
                fprintf(stderr, "-smooth needs a SIGMA > 0 in the units of the spacing (got %s)\n", i + 1 < argc ? argv[i + 1] : "nothing");
                return 2;
            }
            filterSteps.push_back(FilterStep{0, 0u, sigma});
            ++i;
        }
        else if (!strcmp(argv[i], "-show-filtered")) showFiltered = true;
        else if (!strcmp(argv[i], "-thickness")) thickness = true;
        else if (!strcmp(argv[i], "-otsu")) {
            char *e0 = nullptr, *e1 = nullptr, *e2 = nullptr;
            const long k = i + 2 < argc ? strtol(argv[i + 1], &e0, 10) : 0, c = i + 2 < argc ? strtol(argv[i + 2], &e1, 10) : 0;
            if (i + 2 >= argc || e0 == argv[i + 1] || *e0 != '\0' || e1 == argv[i + 2] || *e1 != '\0' || (k != 2 && k != 3) || c < 1 || c > k) {
                fprintf(stderr, "-otsu needs CLASSES = 2 or 3 and CLASS = 1 .. CLASSES (got %s %s)\n", i + 1 < argc ? argv[i + 1] : "nothing", i + 2 < argc ? argv[i + 2] : "nothing");
                return 2;
            }
            otsuClasses = (int)k; otsuClass = (int)c;
            i += 2;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
                const long sh = strtol(argv[i + 1], &e2, 10);
                if (*e2 != '\0' || sh > 15 || (k == 3 && sh < 8)) { fprintf(stderr, "-otsu: SHIFT is 0 .. 15, and at least 8 with three classes (got %s)\n", argv[i + 1]); return 2; }
                otsuShift = (int)sh;
                ++i;
            }
            threshold = true;
        }
        else if (!strcmp(argv[i], "-auto-window")) {
            char *e0 = nullptr, *e1 = nullptr;
            const long lo = i + 2 < argc ? strtol(argv[i + 1], &e0, 10) : 0, hi = i + 2 < argc ? strtol(argv[i + 2], &e1, 10) : 0;
            if (i + 2 >= argc || e0 == argv[i + 1] || *e0 != '\0' || e1 == argv[i + 2] || *e1 != '\0' || lo < 0 || hi > 1000 || lo > hi) {
                fprintf(stderr, "-auto-window needs two quantiles in per mille, 0 <= PLO <= PHI <= 1000 (got %s %s)\n", i + 1 < argc ? argv[i + 1] : "nothing", i + 2 < argc ? argv[i + 2] : "nothing");
                return 2;
            }
            autoLo = (int)lo; autoHi = (int)hi;
            i += 2;
        }
        else if (!strcmp(argv[i], "-threshold")) {
            if (otsuClasses) { fprintf(stderr, "-threshold and -otsu exclude each other\n"); return 2; }
            char *e0 = nullptr, *e1 = nullptr;
            const long lo = i + 2 < argc ? strtol(argv[i + 1], &e0, 10) : 0, hi = i + 2 < argc ? strtol(argv[i + 2], &e1, 10) : 0;
            if (i + 2 >= argc || e0 == argv[i + 1] || *e0 != '\0' || e1 == argv[i + 2] || *e1 != '\0' || lo < 0 || hi > 65535 || lo > hi) {
                fprintf(stderr, "-threshold needs a raw window 0 <= LO <= HI <= 65535 (got %s %s)\n", i + 1 < argc ? argv[i + 1] : "nothing", i + 2 < argc ? argv[i + 2] : "nothing");
                return 2;
            }
            growLo = (int)lo; growHi = (int)hi;
            threshold = true;
            i += 2;
        }
        else if (!strcmp(argv[i], "-fillholes")) cleanSteps.push_back(CleanStep{argv[i], 0, 0u, 0.0});
        else if (!strcmp(argv[i], "-element") && i + 1 < argc) {
            cleanElement = atoi(argv[++i]);
            if (cleanElement != 6 && cleanElement != 18 && cleanElement != 26) { fprintf(stderr, "-element needs 6, 18 or 26 (got %s)\n", argv[i]); return 2; }
        }
        else if (!strcmp(argv[i], "-tf") && i + 1 < argc) tfFile = argv[++i];
        else if (!strcmp(argv[i], "-env") && i + 1 < argc) envFile = argv[++i];
        else if (!strcmp(argv[i], "-frames") && i + 1 < argc) frames = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-depth") && i + 1 < argc) depth = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-size") && i + 2 < argc) { W = atoi(argv[i + 1]); H = atoi(argv[i + 2]); i += 2; }
        else if (!strcmp(argv[i], "-overlay") && i + 2 < argc) {
            overlayFill = atoi(argv[i + 1]); overlayEdge = atoi(argv[i + 2]);
            if (overlayFill < 0 || overlayFill > 255 || overlayEdge < 0 || overlayEdge > 255) { fprintf(stderr, "-overlay needs two opacities 0 .. 255, of the fill and of the outline (got %s %s)\n", argv[i + 1], argv[i + 2]); return 2; }
            overlay = true;
            i += 2;
        }
        else if (!strcmp(argv[i], "-overlay-parts") && i + 1 < argc) {
            overlayParts = atoi(argv[++i]);
            if (overlayParts != 6 && overlayParts != 18 && overlayParts != 26) { fprintf(stderr, "-overlay-parts needs 6, 18 or 26 (got %s)\n", argv[i]); return 2; }
        }
        else if (!strcmp(argv[i], "-raycast")) raycast = true;
        else if (!strcmp(argv[i], "-mip")) { project = true; proj.mode = SVR_PROJ_MIP; }
        else if (!strcmp(argv[i], "-mean")) { project = true; proj.mode = SVR_PROJ_MEAN; }
        else if (!strcmp(argv[i], "-iso") && i + 1 < argc) { project = true; proj.mode = SVR_PROJ_ISO; proj.iso = strtof(argv[++i], nullptr); }
        else if (!strcmp(argv[i], "-slice") && i + 2 < argc) {
            const char* a = argv[i + 1];
            sliceAxis = (a[0] == 'x' || a[0] == 'y' || a[0] == 'z') && a[1] == '\0' ? a[0] - 'x' : -1;
            slicePos = strtof(argv[i + 2], nullptr);
            if (sliceAxis < 0 || !(slicePos >= 0.f && slicePos <= 1.f)) { fprintf(stderr, "-slice needs an axis x, y or z and a position in [0, 1] (got %s %s)\n", a, argv[i + 2]); return 2; }
            i += 2;
        }
        else if (!strcmp(argv[i], "-slab") && i + 2 < argc) {
            slabThickness = strtof(argv[i + 1], nullptr);
            const char* m = argv[i + 2];
            slabMode = !strcmp(m, "mip") ? SVR_SLAB_MIP : !strcmp(m, "minip") ? SVR_SLAB_MINIP : !strcmp(m, "mean") ? SVR_SLAB_MEAN : 0;
            if (!(slabThickness > 0.f) || !slabMode) { fprintf(stderr, "-slab needs a thickness > 0 and mip, minip or mean (got %s %s)\n", argv[i + 1], m); return 2; }
            i += 2;
        }
        else if (!strcmp(argv[i], "-stack") && i + 1 < argc) {
            stack = atoi(argv[++i]);
            if (stack < 1 || stack > 9999) { fprintf(stderr, "-stack needs 1 .. 9999 slices (got %s)\n", argv[i]); return 2; }
        }
        else if (!strcmp(argv[i], "-pick") && i + 2 < argc) {
            const int px = atoi(argv[i + 1]), py = atoi(argv[i + 2]);
            if (px < 0 || py < 0 || picks.size() >= 2u * SVR_PICK_MAX) { fprintf(stderr, "-pick needs a pixel X Y >= 0, at most %d of them (got %s %s)\n", SVR_PICK_MAX, argv[i + 1], argv[i + 2]); return 2; }
            picks.push_back((uint32_t)px); picks.push_back((uint32_t)py);
            i += 2;
        }
        else if (!strcmp(argv[i], "-grow") && i + 4 < argc) {
            growX = atoi(argv[i + 1]); growY = atoi(argv[i + 2]); growLo = atoi(argv[i + 3]); growHi = atoi(argv[i + 4]);
            if (growX < 0 || growY < 0 || growLo < 0 || growHi > 65535 || growLo > growHi) { fprintf(stderr, "-grow needs a pixel X Y >= 0 and a raw window 0 <= LO <= HI <= 65535 (got %s %s %s %s)\n", argv[i + 1], argv[i + 2], argv[i + 3], argv[i + 4]); return 2; }
            grow = true;
            i += 4;
        }
        else if (!strcmp(argv[i], "-seed") && i + 3 < argc) {
            SeedStroke s = {atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), -1.0};
            if (s.x < 0 || s.y < 0 || s.cls < 1 || s.cls > (int)Canvas::SEED_MAX_CLASS) { fprintf(stderr, "-seed needs a pixel X Y >= 0 and a class 1 .. %u (got %s %s %s)\n", Canvas::SEED_MAX_CLASS, argv[i + 1], argv[i + 2], argv[i + 3]); return 2; }
            i += 3;
            char* end = nullptr;
            if (i + 1 < argc && argv[i + 1][0] != '-' && (s.radius = strtod(argv[i + 1], &end), end != argv[i + 1] && !*end)) {
                if (!(s.radius >= 0.0) || !std::isfinite(s.radius)) { fprintf(stderr, "-seed: the brush radius must be >= 0, in the units of the spacing (got %s)\n", argv[i + 1]); return 2; }
                ++i;
            }
            else s.radius = -1.0;
            seeds.push_back(s);
        }
        else if (!strcmp(argv[i], "-growcut")) {
            growcut = true;
            if (i + 2 < argc && argv[i + 1][0] != '-' && argv[i + 2][0] != '-') {
                growGain = atoi(argv[i + 1]); growShift = atoi(argv[i + 2]);
                if (growGain < 0 || growGain > 65535 || growShift < 0 || growShift > 15) { fprintf(stderr, "-growcut needs GAIN 0 .. 65535 and SHIFT 0 .. 15 (got %s %s)\n", argv[i + 1], argv[i + 2]); return 2; }
                i += 2;
            }
        }
        else if (!strcmp(argv[i], "-keep-class") && i + 1 < argc) {
            keepClass = atoi(argv[++i]);
            if (keepClass < 1 || keepClass > (int)Canvas::SEED_MAX_CLASS) { fprintf(stderr, "-keep-class needs a class 1 .. %u (got %s)\n", Canvas::SEED_MAX_CLASS, argv[i]); return 2; }
        }
        else if (!strcmp(argv[i], "-conn") && i + 1 < argc) {
            growConn = atoi(argv[++i]);
            if (growConn != 6 && growConn != 18 && growConn != 26) { fprintf(stderr, "-conn needs 6, 18 or 26 (got %s)\n", argv[i]); return 2; }
        }
        else if (!strcmp(argv[i], "-keep")) growMode = SVR_REGION_KEEP;
        else if (!strcmp(argv[i], "-remove")) growMode = SVR_REGION_REMOVE;
        else if (!strcmp(argv[i], "-hit") && i + 1 < argc) {
            const char* m = argv[++i];
            if (!strcmp(m, "max")) hitParams.mode = SVR_HIT_MAX;
            else if (!strcmp(m, "opacity") && i + 1 < argc) { hitParams.mode = SVR_HIT_OPACITY; hitParams.alpha = strtof(argv[++i], nullptr); }
            else if (!strcmp(m, "iso") && i + 1 < argc) { hitParams.mode = SVR_HIT_ISO; hitParams.iso = strtof(argv[++i], nullptr); }
            else { fprintf(stderr, "-hit needs opacity A, iso L or max (got %s)\n", m); return 2; }
        }
        else if (!strcmp(argv[i], "-window") && i + 2 < argc) { proj.window_lo = strtof(argv[i + 1], nullptr); proj.window_hi = strtof(argv[i + 2], nullptr); i += 2; }
        else if (!strcmp(argv[i], "-tfcolor")) proj.flags |= SVR_PROJ_COLOR_TF;
        else if (!strcmp(argv[i], "-denoise-preview") && i + 1 < argc) denoisePreview = atoi(argv[++i]);   // denoised image up to N spp
        else if (!strcmp(argv[i], "-noise") && i + 1 < argc) {                                          // render until converged
            char* end = nullptr;
            noiseTarget = strtof(argv[++i], &end);
            if (end == argv[i] || *end != '\0' || !(noiseTarget > 0.f)) { fprintf(stderr, "-noise needs a target RMSE > 0 (got %s)\n", argv[i]); return 2; }
        }
        else if (!strcmp(argv[i], "-adaptive") && i + 1 < argc) {                                       // adaptive sampling
            char* end = nullptr;
            adaptiveTarget = strtof(argv[++i], &end);
            if (end == argv[i] || *end != '\0' || !(adaptiveTarget > 0.f)) { fprintf(stderr, "-adaptive needs a tile target RMSE > 0 (got %s)\n", argv[i]); return 2; }
        }
        else if (!strcmp(argv[i], "-mesh")) {
            if (i + 1 >= argc || !meshName(argv[i + 1])) { fprintf(stderr, "-mesh needs a file name that ends in .stl or .ply (got %s)\n", i + 1 < argc ? argv[i + 1] : "nothing"); return 2; }
            meshFile = argv[++i];
        }
        else if (!strcmp(argv[i], "-relax")) {
            char* end = nullptr;
            const long v = i + 1 < argc ? strtol(argv[i + 1], &end, 10) : -1;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || v < 0 || v > SVR_MESH_MAX_RELAX) { fprintf(stderr, "-relax needs a number of steps N in 0 .. %d (got %s)\n", SVR_MESH_MAX_RELAX, i + 1 < argc ? argv[i + 1] : "nothing"); return 2; }
            meshRelax = (int)v;
            ++i;
        }
        else if (!strcmp(argv[i], "-mesh-iso")) {
            char* end = nullptr;
            const long v = i + 2 < argc ? strtol(argv[i + 1], &end, 10) : 0;
            if (i + 2 >= argc || end == argv[i + 1] || *end != '\0' || v < 1 || v > 65535 || !meshName(argv[i + 2])) {
                fprintf(stderr, "-mesh-iso needs a raw level 1 .. 65535 and a file name that ends in .stl or .ply (got %s %s)\n", i + 1 < argc ? argv[i + 1] : "nothing", i + 2 < argc ? argv[i + 2] : "nothing");
                return 2;
            }
            meshIsoLevel = (int)v;
            meshIsoFile = argv[i + 2];
            i += 2;
        }
        else if (!strcmp(argv[i], "-crop")) {
            GridStep g = {true, {0, 0, 0}, {0, 0, 0}, 0.0, SVR_RESAMPLE_NEAREST};
            bool ok = i + 6 < argc;
            for (int k = 0; ok && k < 6; ++k) {
                char* end = nullptr;
                const long v = strtol(argv[i + 1 + k], &end, 10);
                ok = end != argv[i + 1 + k] && *end == '\0' && v >= -0x7fffffffL && v <= 0x7fffffffL;
                (k < 3 ? g.lo[k] : g.hi[k - 3]) = (int32_t)v;
            }
            if (!ok) { fprintf(stderr, "-crop needs an inclusive voxel box X0 Y0 Z0 X1 Y1 Z1\n"); return 2; }
            gridSteps.push_back(g);
            i += 6;
        }
        else if (!strcmp(argv[i], "-resample")) {
            char* end = nullptr;
            const double mm = i + 1 < argc ? strtod(argv[i + 1], &end) : 0.0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(mm > 0.0) || !std::isfinite(mm)) {
                fprintf(stderr, "-resample needs a spacing MM > 0 in the units of the file's spacing (got %s)\n", i + 1 < argc ? argv[i + 1] : "nothing");
                return 2;
            }
            GridStep g = {false, {0, 0, 0}, {0, 0, 0}, mm, SVR_RESAMPLE_AUTO};
            ++i;
            const char* m = i + 1 < argc ? argv[i + 1] : "";
            const int mode = !strcmp(m, "nearest") ? SVR_RESAMPLE_NEAREST : !strcmp(m, "linear") ? SVR_RESAMPLE_LINEAR : !strcmp(m, "area") ? SVR_RESAMPLE_AREA
                           : !strcmp(m, "auto") ? SVR_RESAMPLE_AUTO : -1;
            if (mode >= 0) { g.mode = mode; ++i; }
            gridSteps.push_back(g);
        }
        else if (!strcmp(argv[i], "-save-volume") || !strcmp(argv[i], "-save-mask") || !strcmp(argv[i], "-save-parts")) {
            if (i + 1 >= argc || argv[i + 1][0] == '-') { fprintf(stderr, "%s needs a file name (.mhd or .mha)\n", argv[i]); return 2; }
            (argv[i][6] == 'v' ? saveVolumeFile : argv[i][6] == 'm' ? saveMaskFile : savePartsFile) = argv[i + 1];
            ++i;
        }
        else if (!strcmp(argv[i], "-compare-mask")) {
            if (i + 1 >= argc || argv[i + 1][0] == '-') { fprintf(stderr, "-compare-mask needs the file name of a mask (.mhd or .mha, one byte per voxel)\n"); return 2; }
            compareMaskFile = argv[++i];
        }
        else if (!strcmp(argv[i], "-scissor") || !strcmp(argv[i], "-scissor-slice")) {
            const bool onSlice = argv[i][8] != '\0';
            const char* const name = argv[i];
            ScissorStep sc = {-1, 0.5f, 0, 0.f, {}};
            bool ok = true;
            if (onSlice) {
                ok = i + 2 < argc;
                if (ok) {
                    const char* a = argv[i + 1];
                    sc.axis = (!strcmp(a, "x") || !strcmp(a, "0")) ? 0 : (!strcmp(a, "y") || !strcmp(a, "1")) ? 1 : (!strcmp(a, "z") || !strcmp(a, "2")) ? 2 : -1;
                    sc.pos = (float)atof(argv[i + 2]);
                    ok = sc.axis >= 0 && sc.pos >= 0.f && sc.pos <= 1.f;
                    i += 2;
                }
            }
            ok = ok && i + 1 < argc;
            if (ok) {
                const char* o = argv[++i];
                sc.op = !strcmp(o, "inside") ? SVR_SCISSOR_ERASE_INSIDE : !strcmp(o, "outside") ? SVR_SCISSOR_ERASE_OUTSIDE : (onSlice && !strcmp(o, "fill")) ? SVR_SCISSOR_FILL_INSIDE : 0;
                ok = sc.op != 0;
            }
            if (ok && onSlice) {
                char* end = nullptr;
                sc.thickness = i + 1 < argc ? strtof(argv[i + 1], &end) : -1.f;
                ok = i + 1 < argc && end != argv[i + 1] && *end == '\0' && sc.thickness >= 0.f && std::isfinite(sc.thickness);
                ++i;
            }
            while (ok && i + 1 < argc) {                            // the coordinates: every following argument that is a number
                char* end = nullptr;
                const double v = strtod(argv[i + 1], &end);
                if (end == argv[i + 1] || *end != '\0') break;
                sc.polygon.push_back(v);
                ++i;
            }
            if (!ok || sc.polygon.size() < 4 || sc.polygon.size() % 2 != 0) {
                fprintf(stderr, "%s needs %sinside|outside%s and the points X0 Y0 X1 Y1 [X2 Y2 ...] in pixels: two corners of a rectangle, or three or more vertices\n", name,
                        onSlice ? "an axis x, y or z, a position in [0, 1], " : "", onSlice ? "|fill, a slab thickness >= 0" : "");
                return 2;
            }
            if (sc.polygon.size() == 4) {                           // two corners: the inclusive pixel rectangle
                int32_t q[8];
                const double x0 = std::fmin(sc.polygon[0], sc.polygon[2]), x1 = std::fmax(sc.polygon[0], sc.polygon[2]);
                const double y0 = std::fmin(sc.polygon[1], sc.polygon[3]), y1 = std::fmax(sc.polygon[1], sc.polygon[3]);
                if (!(std::fabs(x0) < 4e4 && std::fabs(x1) < 4e4 && std::fabs(y0) < 4e4 && std::fabs(y1) < 4e4) ||
                    svr_stencil_rect((int32_t)std::floor(x0), (int32_t)std::floor(y0), (int32_t)std::floor(x1), (int32_t)std::floor(y1), q) != 0) {
                    fprintf(stderr, "%s: the rectangle lies beyond the coordinate limit\n", name);
                    return 2;
                }
                sc.polygon.clear();
                for (int k = 0; k < 8; ++k) sc.polygon.push_back(q[k] / 256.0);
            }
            scissorSteps.push_back(sc);
        }
        else if (!strcmp(argv[i], "-fill-between")) {
            const char* a = i + 1 < argc ? argv[i + 1] : "";
            fillBetweenAxis = (!strcmp(a, "x") || !strcmp(a, "0")) ? 0 : (!strcmp(a, "y") || !strcmp(a, "1")) ? 1 : (!strcmp(a, "z") || !strcmp(a, "2")) ? 2 : -1;
            if (fillBetweenAxis < 0) { fprintf(stderr, "-fill-between needs an axis x, y or z\n"); return 2; }
            ++i;
        }
        else if (!strcmp(argv[i], "-smooth-region")) {
            const char* a = i + 1 < argc ? argv[i + 1] : "";
            smoothRegionOp = !strcmp(a, "median") ? SVR_SMOOTH_MAJORITY : !strcmp(a, "gauss") ? SVR_SMOOTH_BINOMIAL : 0;
            if (!smoothRegionOp || i + 2 >= argc || !sizeArg(argv[i + 2], &smoothRegionSize)) { fprintf(stderr, "-smooth-region needs median or gauss and a SIZE >= 0 in the units of the spacing\n"); return 2; }
            i += 2;
            if (!timesArg(&i, &smoothRegionN)) { fprintf(stderr, "-smooth-region: N must lie in 1 .. %d\n", SVR_REGION_SMOOTH_MAX_ITERATIONS); return 2; }
        }
        else if (!strcmp(argv[i], "-smooth-parts")) {
            if (i + 1 >= argc || !sizeArg(argv[i + 1], &smoothPartsSize)) { fprintf(stderr, "-smooth-parts needs a SIZE >= 0 in the units of the spacing\n"); return 2; }
            ++i;
            if (!timesArg(&i, &smoothPartsN)) { fprintf(stderr, "-smooth-parts: N must lie in 1 .. %d\n", SVR_REGION_SMOOTH_MAX_ITERATIONS); return 2; }
        }
        else if (!strcmp(argv[i], "-density")) {
            if (i + 1 >= argc || !sizeArg(argv[i + 1], &densitySize)) { fprintf(stderr, "-density needs a SIZE >= 0 in the units of the spacing\n"); return 2; }
            ++i;
        }
        else if (!strcmp(argv[i], "-save-crop")) {
            char* end = nullptr;
            const long v = i + 3 < argc ? strtol(argv[i + 3], &end, 10) : -1;
            if (i + 3 >= argc || end == argv[i + 3] || *end != '\0' || v < 0 || v > 0x7fffffffL) {
                fprintf(stderr, "-save-crop needs two file names, of the voxels and of the mask, and a margin in voxels >= 0\n");
                return 2;
            }
            saveCropVolume = argv[i + 1]; saveCropMask = argv[i + 2]; saveCropMargin = (int)v;
            i += 3;
        }
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) out = argv[++i];
        else { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
    }
    if ((slabMode || stack) && sliceAxis < 0) { fprintf(stderr, "-slab and -stack need -slice\n"); return 2; }
    if (grow && threshold) { fprintf(stderr, "-grow and -threshold / -otsu exclude each other\n"); return 2; }
    if (autoLo >= 0 && sliceAxis < 0 && !(project && proj.mode != SVR_PROJ_ISO)) { fprintf(stderr, "-auto-window sets the grey window of -slice, -mip or -mean\n"); return 2; }
    if (growcut && seeds.empty()) { fprintf(stderr, "-growcut needs strokes: -seed X Y CLASS [RADIUS], at least one\n"); return 2; }
    if (!seeds.empty() && !growcut) { fprintf(stderr, "-seed needs -growcut [GAIN SHIFT]\n"); return 2; }
    if (keepClass && !growcut) { fprintf(stderr, "-keep-class needs -growcut [GAIN SHIFT]\n"); return 2; }
    const bool anyRegion = grow || threshold || growcut;           // something makes a region: the steps after it have one to work on
    if (!cleanSteps.empty() && !anyRegion) {
        if (cleanSteps[0].op <= -3) fprintf(stderr, "%s needs -grow X Y LO HI or -threshold LO HI\n", cleanSteps[0].name);
        else fprintf(stderr, "%s needs -grow X Y LO HI\n", cleanSteps[0].name);
        return 2;
    }
    if (thickness && !anyRegion) { fprintf(stderr, "-thickness needs -grow X Y LO HI or -threshold LO HI\n"); return 2; }
    if (!grow)
        for (const CleanStep& c : cleanSteps)
            if (c.op == -1) { fprintf(stderr, "-detach starts from the picked voxel: it needs -grow X Y LO HI, not -threshold\n"); return 2; }
    if ((overlay || overlayParts) && !anyRegion) { fprintf(stderr, "-overlay needs a region: -grow X Y LO HI or -threshold LO HI\n"); return 2; }
    if (overlayParts && !overlay) { fprintf(stderr, "-overlay-parts needs -overlay FILL EDGE\n"); return 2; }
    if (overlay && sliceAxis < 0 && !raycast && !(project && proj.mode != SVR_PROJ_MEAN)) { fprintf(stderr, "-overlay tints a slice or a picture with one hit per pixel: it needs -slice, -stack, -raycast, -mip or -iso L\n"); return 2; }
    if (!meshFile.empty() && !anyRegion) { fprintf(stderr, "-mesh exports the surface of a region: it needs -grow X Y LO HI or -threshold LO HI\n"); return 2; }
    if (meshRelax >= 0 && meshFile.empty()) { fprintf(stderr, "-relax needs -mesh FILE\n"); return 2; }
    if (showFiltered && filterSteps.empty()) { fprintf(stderr, "-show-filtered needs -median E N or -smooth SIGMA\n"); return 2; }
    if ((!saveMaskFile.empty() || !savePartsFile.empty() || !saveCropVolume.empty()) && !anyRegion) {
        fprintf(stderr, "-save-mask, -save-parts and -save-crop write a region: they need -grow X Y LO HI or -threshold LO HI\n");
        return 2;
    }
    if (!scissorSteps.empty() && !anyRegion) { fprintf(stderr, "-scissor and -scissor-slice cut a region: they need -grow X Y LO HI or -threshold LO HI\n"); return 2; }
    if (fillBetweenAxis >= 0 && !anyRegion) { fprintf(stderr, "-fill-between fills a region: it needs -grow X Y LO HI or -threshold LO HI\n"); return 2; }
    if ((smoothRegionOp || smoothPartsSize >= 0.0 || densitySize >= 0.0) && !anyRegion) { fprintf(stderr, "-smooth-region, -smooth-parts and -density work on a region: they need -grow X Y LO HI, -threshold LO HI or -growcut\n"); return 2; }
    if (!compareMaskFile.empty() && !anyRegion) { fprintf(stderr, "-compare-mask compares a region with the file: it needs -grow X Y LO HI or -threshold LO HI\n"); return 2; }
    if (svr_init(0)) return 1;
    {
        Canvas canvas(W, H);

        // MainWindow::MainWindow, mainwindow.cpp:22-62: default opacity ramp and colour map, or a saved configuration
        TransferFunction tf;
        if (!tfFile.empty()) {
            if (!tf.LoadExistingTFConfiguration(tfFile)) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
        } else {
            tf.AddPoint(0.0, 0.0);
            for (int i = 1; i <= 10; ++i) tf.AddPoint(0.1 * i, 0.5);
            tf.AddRGBPoint(0.0, 69 / 255.0, 199 / 255.0, 186 / 255.0);
            tf.AddRGBPoint(0.2, 172 / 255.0, 3 / 255.0, 57 / 255.0);
            tf.AddRGBPoint(0.4, 169 / 255.0, 83 / 255.0, 58 / 255.0);
            tf.AddRGBPoint(0.6, 43 / 255.0, 32 / 255.0, 161 / 255.0);
            tf.AddRGBPoint(0.8, 247 / 255.0, 158 / 255.0, 97 / 255.0);
            tf.AddRGBPoint(1.0, 183 / 255.0, 7 / 255.0, 140 / 255.0);
        }
        const cudaTextureObject_t tfTex = tf.Update();                // (argument evaluation order is unspecified)
        canvas.SetTransferFunction(tfTex, tf.GetMaxOpacityValue());

        canvas.volumeReader->KeepVoxels(anyRegion || autoLo >= 0 || !filterSteps.empty() || !meshIsoFile.empty() || !gridSteps.empty() ||
                                        !saveVolumeFile.empty());    // the region, filter, grid and save calls work on the plain voxels
        canvas.LoadVolume(volume);
        if (!canvas.volumeReader->IsLoaded()) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
        printf("%s: %d x %d x %d, range %.0f..%.0f, max gradient magnitude %.0f, %zu histogram bins\n", volume.c_str(),
               canvas.volumeReader->dim[0], canvas.volumeReader->dim[1], canvas.volumeReader->dim[2], canvas.volumeReader->range[0],
               canvas.volumeReader->range[1], canvas.volumeReader->maxMagnitude, canvas.volumeReader->histogram.size());
        for (const GridStep& g : gridSteps) {
            // the grid everything after works on
            const double target[3] = {g.mm, g.mm, g.mm};
            if ((g.crop ? canvas.CropVolume(g.lo, g.hi) : canvas.ResampleVolume(target, g.mode)) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
            float ms = 0.f;
            svr_volume_resample_last_ms(&ms);
            const int* d = canvas.volumeReader->dim;
            const char* modes[] = {"nearest", "linear", "area", "auto"};
            if (g.crop) printf("crop %d %d %d .. %d %d %d: ", g.lo[0], g.lo[1], g.lo[2], g.hi[0], g.hi[1], g.hi[2]);
            else printf("resample %g %s: ", g.mm, modes[g.mode]);
            printf("%d x %d x %d, spacing %.9g %.9g %.9g, %.3f ms\n", d[0], d[1], d[2], canvas.Volume().spacing.x, canvas.Volume().spacing.y, canvas.Volume().spacing.z, ms);
        }
        // a file that a -save-* step wrote: its dimensions, the spacing and the time, write included
        const auto saved = [&](const char* what, const std::string& file, const int32_t d[3], const std::chrono::steady_clock::time_point& t0) {
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            printf("%s -> %s: %d x %d x %d, spacing %.9g %.9g %.9g, %.3f ms\n", what, file.c_str(), d[0], d[1], d[2], canvas.Volume().spacing.x, canvas.Volume().spacing.y,
                   canvas.Volume().spacing.z, ms);
        };

        // the "add light" dialog's defaults (mainwindow.cpp:229-238): a disk above the volume, facing down
        cudaAreaLight light;
        float dist = canvas.volumeReader->GetBoundingSphereRadius() * 1.5f + 1.f;
        light.Set(cudaDisk(glm::vec3(0.f, dist, 0.f), glm::vec3(0.f, -1.f, 0.f), 10.f), glm::vec3(1.f), 500.f);
        canvas.lights.AddAreaLights(light, glm::vec3(0.f, 0.f, dist));
        canvas.SetAreaLights();
        if (!envFile.empty()) {
            canvas.SetEnvLightMap(envFile);
            svr_set_option(SVR_OPT_ENV_ON_ESCAPE, 1);
        }
        canvas.SetScatterTimes(depth);
        canvas.SetRenderMode(project ? RENDER_MODE_PROJECTION : (raycast ? RENDER_MODE_RAYCASTING : RENDER_MODE_PATHTRACER));
        canvas.SetProjection(proj);
        raycast = raycast || project;                                  // one deterministic image either way
        canvas.SetDenoisePreview(denoisePreview);

        for (const FilterStep& f : filterSteps) {
            // filter the voxels that -grow / -threshold will segment
            float ms = 0.f;
            if (f.element) {
                if (canvas.MedianVolume(f.element, f.iterations) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                svr_volume_filter_last_ms(&ms);
                printf("median element %d x %u: %.3f ms\n", f.element, f.iterations, ms);
            } else {
                const double sp[3] = {canvas.Volume().spacing.x, canvas.Volume().spacing.y, canvas.Volume().spacing.z};
                uint32_t radii[3] = {0u, 0u, 0u};
                double applied[3] = {0.0, 0.0, 0.0};
                if (svr_volume_smooth_radii(sp, f.sigma, radii, applied) != 0 || canvas.SmoothVolume(f.sigma) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                svr_volume_filter_last_ms(&ms);
                printf("smooth sigma %g: radii %u %u %u (sigma %g %g %g), %.3f ms\n", f.sigma, radii[0], radii[1], radii[2], applied[0], applied[1], applied[2], ms);
            }
        }
        if (showFiltered && canvas.ShowFiltered() != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
        if (autoLo >= 0) {
            // the grey window of the slice or projection from two quantiles of the voxels
            uint32_t raw[2] = {0u, 0u};
            if (canvas.AutoWindow((uint32_t)autoLo, (uint32_t)autoHi, 1000u, &proj.window_lo, &proj.window_hi, false, raw) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
            float ms = 0.f;
            svr_volume_histogram_last_ms(&ms);
            printf("auto-window %d %d: raw %u..%u, window %.9g %.9g; %.3f ms\n", autoLo, autoHi, raw[0], raw[1], proj.window_lo, proj.window_hi, ms);
            canvas.SetProjection(proj);
        }
        if (!saveVolumeFile.empty()) {
            const auto t0 = std::chrono::steady_clock::now();
            if (canvas.SaveVolume(saveVolumeFile) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
            saved("save-volume", saveVolumeFile, canvas.volumeReader->dim, t0);
        }

        // an extracted surface goes to its file in world coordinates, with one line of counts and measures in the spacing's units
        const auto exportSurface = [&](const std::string& file) {
            double vol = 0.0, area = 0.0;
            if (canvas.SurfaceMeasure(&vol, &area) != 0 || canvas.SaveSurface(file) != 0) return false;
            printf("mesh: %zu vertices, %zu triangles, volume %.9g mm^3, area %.9g mm^2\n", canvas.SurfaceVertices().size() / 3, canvas.SurfaceTriangles().size() / 3, vol, area);
            return true;
        };

        if (!picks.empty()) {
            // point picks instead of a rendering: one line per pick
            const uint32_t n = (uint32_t)(picks.size() / 2);
            std::vector<svr_hit> hits(n);
            void* d = svr_device_malloc(n * sizeof(svr_hit));
            if (!d) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
            int rc = svr_pick(d, picks.data(), n, &canvas.Volume(), &canvas.TransferFunctionPod(), &canvas.Camera(),
                              canvas.volumeReader->GetElementBoundingSphereRadius(), &hitParams);
            if (rc == 0) rc = svr_memcpy_d2h(hits.data(), d, n * sizeof(svr_hit));
            svr_device_free(d);
            if (rc != 0 || svr_last_error_code()) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
            for (uint32_t i = 0; i < n; ++i) {
                const svr_hit& hh = hits[i];
                if (hh.status == SVR_HIT_STATUS_FOUND)
                    printf("pick %u %u: hit at sample %d, t %g, value %g, position %g %g %g, normal %g %g %g\n", picks[2 * i], picks[2 * i + 1], hh.sample, hh.t, hh.value,
                           hh.position.x, hh.position.y, hh.position.z, hh.normal.x, hh.normal.y, hh.normal.z);
                else
                    printf("pick %u %u: %s\n", picks[2 * i], picks[2 * i + 1], hh.status == SVR_HIT_STATUS_MISS ? "the ray misses the volume" : "no hit along the ray");
            }
            svr_shutdown();
            return 0;
        }

        if (anyRegion) {
            // pick, segment, measure; what follows renders the kept (or the remaining) volume
            svr_hit hit = svr_hit();
            svr_region_stats st = svr_region_stats();
            const double sp[3] = {canvas.Volume().spacing.x, canvas.Volume().spacing.y, canvas.Volume().spacing.z};
            svr_region_measurement m = svr_region_measurement();
            if (grow || threshold) {
                if (grow && canvas.Pick((uint32_t)growX, (uint32_t)growY, &hit, hitParams) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                if (grow && hit.status != SVR_HIT_STATUS_FOUND) { fprintf(stderr, "-grow: %s at pixel %d %d\n", hit.status == SVR_HIT_STATUS_MISS ? "the ray misses the volume" : "no hit along the ray", growX, growY); return 1; }
                if (otsuClasses) {
                    uint32_t thr[2] = {0u, 0u}, win[2] = {0u, 0u};
                    if (canvas.OtsuRegion((uint32_t)otsuClasses, (uint32_t)otsuClass, (uint32_t)otsuShift, &st, thr, win) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                    growLo = (int)win[0]; growHi = (int)win[1];
                    if (otsuClasses == 2) printf("otsu 2 classes shift %d: threshold %u; class %d window %d..%d\n", otsuShift, thr[0], otsuClass, growLo, growHi);
                    else printf("otsu 3 classes shift %d: thresholds %u %u; class %d window %d..%d\n", otsuShift, thr[0], thr[1], otsuClass, growLo, growHi);
                }
                else if ((grow ? canvas.GrowRegion(hit, (uint32_t)growLo, (uint32_t)growHi, growConn, &st) : canvas.ThresholdRegion((uint32_t)growLo, (uint32_t)growHi, &st)) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                if (svr_region_measure(&st, sp, &m) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                if (threshold) {
                    uint32_t parts = 0u;
                    if (canvas.CountRegionParts(growConn, &parts) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                    if (st.status == SVR_REGION_STATUS_EMPTY)
                        printf("threshold window %d..%d: no voxel lies in the window; the region is empty\n", growLo, growHi);
                    else
                        printf("threshold window %d..%d conn %d: %u parts, %llu voxels, volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g\n",
                               growLo, growHi, growConn, parts, (unsigned long long)st.voxels, m.volume, m.mean, m.stddev, st.vmin, st.vmax, st.bbox_min[0], st.bbox_min[1],
                               st.bbox_min[2], st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area);
                }
                else if (st.status == SVR_REGION_STATUS_EMPTY)
                    printf("grow %d %d window %d..%d: the picked voxel (value %g) is outside the window; the region is empty\n", growX, growY, growLo, growHi, hit.value);
                else
                    printf("grow %d %d window %d..%d conn %d: %llu voxels, volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g; %u sweeps\n",
                           growX, growY, growLo, growHi, growConn, (unsigned long long)st.voxels, m.volume, m.mean, m.stddev, st.vmin, st.vmax, st.bbox_min[0], st.bbox_min[1],
                           st.bbox_min[2], st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area, st.sweeps);
                if (st.status != SVR_REGION_STATUS_EMPTY) {
                    uint32_t median = 0u;
                    if (canvas.RegionMedian(&median) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                    printf("median: raw %u\n", median);
                }
            }
            const auto smoothParts = [&](const char* what) {          // -smooth-parts on the canvas's label map
                uint64_t changed = 0u;
                if (canvas.SmoothRegionParts(smoothPartsSize, (uint32_t)smoothPartsN, &changed) != 0) {
                    fprintf(stderr, "-smooth-parts: %s\n", svr_last_error_code() ? svr_last_error() : "more than 255 parts, or none");
                    return false;
                }
                float ms = 0.f;
                svr_region_smooth_last_ms(&ms);
                printf("smooth-parts %g x %d (%s): %llu voxels changed their part; %.3f ms\n", smoothPartsSize, smoothPartsN, what, (unsigned long long)changed, ms);
                partsSmoothed = true;
                return true;
            };
            if (growcut) {
                // strokes of classes on picked voxels, grown over the region made above or, without one, over the whole volume
                const double brush = 2.0 * std::fmin(sp[0], std::fmin(sp[1], sp[2]));
                for (const SeedStroke& s : seeds) {
                    svr_hit sh = svr_hit();
                    if (canvas.Pick((uint32_t)s.x, (uint32_t)s.y, &sh, hitParams) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                    if (sh.status != SVR_HIT_STATUS_FOUND) { fprintf(stderr, "-seed: %s at pixel %d %d\n", sh.status == SVR_HIT_STATUS_MISS ? "the ray misses the volume" : "no hit along the ray", s.x, s.y); return 1; }
                    if (canvas.AddSeed(sh, (uint32_t)s.cls, s.radius < 0.0 ? brush : s.radius) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                }
                svr_growcut_params gp;
                svr_region_growcut_params_default(&gp, 26);
                gp.contrast_gain = (uint32_t)growGain; gp.contrast_shift = (uint32_t)growShift;
                uint32_t found = 0u;
                const int rc = canvas.GrowFromSeeds(&gp, grow || threshold, &found);
                if (rc != 0 && rc != SVR_REGION_ERR_RANGE) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                float ms = 0.f;
                svr_region_growcut_last_ms(&ms);
                printf("growcut gain %d shift %d, %zu strokes%s: %u classes own voxels; %.2f ms%s\n", growGain, growShift, seeds.size(),
                       grow || threshold ? " inside the region" : "", found, ms, rc ? "; COSTS SATURATED: raise SHIFT or lower GAIN" : "");
                if (smoothPartsSize >= 0.0 && !smoothParts("the classes of -growcut")) return 1;
                if (keepClass) {
                    partsSmoothed = false;
                    if (canvas.KeepSeedClass((uint32_t)keepClass, &st) != 0 || svr_region_measure(&st, sp, &m) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                    if (st.status == SVR_REGION_STATUS_EMPTY)
                        printf("keep-class %d: the region is empty\n", keepClass);
                    else
                        printf("keep-class %d: %llu voxels, volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g\n", keepClass,
                               (unsigned long long)st.voxels, m.volume, m.mean, m.stddev, st.vmin, st.vmax, st.bbox_min[0], st.bbox_min[1], st.bbox_min[2],
                               st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area);
                }
            }
            if (!cleanSteps.empty()) {
                std::string done;
                bool plainSteps = false;                           // a step other than -largest / -minsize / -ball-* / -split: those print their own lines
                for (const CleanStep& c : cleanSteps) {
                    if (c.op <= -10) {
                        uint32_t w[3] = {0u, 0u, 0u};
                        double unit = 0.0;
                        int rc = canvas.RegionDistanceUnits(w, &unit);
                        if (rc == 0) rc = canvas.BallMorphRegion(-10 - c.op, c.length, &st);
                        if (rc == 0) rc = svr_region_measure(&st, sp, &m);
                        if (rc != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                        if (st.status == SVR_REGION_STATUS_EMPTY)
                            printf("%s %g (unit %g, weights %u %u %u): the region is empty\n", c.name + 1, c.length, unit, w[0], w[1], w[2]);
                        else
                            printf("%s %g (unit %g, weights %u %u %u): %llu voxels, volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g\n",
                                   c.name + 1, c.length, unit, w[0], w[1], w[2], (unsigned long long)st.voxels, m.volume, m.mean, m.stddev, st.vmin, st.vmax, st.bbox_min[0],
                                   st.bbox_min[1], st.bbox_min[2], st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area);
                        char len[32];
                        snprintf(len, sizeof len, "%g", c.length);
                        done += std::string(done.empty() ? "" : " ") + (c.name + 1) + " " + len;
                        continue;
                    }
                    if (c.op == -5) {
                        uint32_t parts = 0u;
                        int rc = canvas.SplitRegion(c.length, growConn, &parts, &st);
                        if (rc == 0) rc = svr_region_measure(&st, sp, &m);
                        if (rc != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                        if (st.status == SVR_REGION_STATUS_EMPTY)
                            printf("split %g conn %d: %u parts; the region is empty\n", c.length, growConn, parts);
                        else
                            printf("split %g conn %d: %u parts, %llu voxels, volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g\n",
                                   c.length, growConn, parts, (unsigned long long)st.voxels, m.volume, m.mean, m.stddev, st.vmin, st.vmax, st.bbox_min[0], st.bbox_min[1],
                                   st.bbox_min[2], st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area);
                        char len[32];
                        snprintf(len, sizeof len, "%g", c.length);
                        done += std::string(done.empty() ? "" : " ") + "split " + len;
                        continue;
                    }
                    if (c.op <= -3) {
                        uint32_t before = 0u, after = 0u;
                        int rc = canvas.CountRegionParts(growConn, &before);
                        if (rc == 0) rc = c.op == -3 ? canvas.KeepLargestRegion((int)c.radius, growConn, &st) : canvas.RemoveSmallRegions(c.radius, growConn, &st);
                        if (rc == 0) rc = canvas.CountRegionParts(growConn, &after);
                        if (rc == 0) rc = svr_region_measure(&st, sp, &m);
                        if (rc != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                        if (st.status == SVR_REGION_STATUS_EMPTY)
                            printf("%s %u conn %d: %u of %u parts kept; the region is empty\n", c.name + 1, c.radius, growConn, after, before);
                        else
                            printf("%s %u conn %d: %u of %u parts kept, %llu voxels, volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g\n",
                                   c.name + 1, c.radius, growConn, after, before, (unsigned long long)st.voxels, m.volume, m.mean, m.stddev, st.vmin, st.vmax, st.bbox_min[0],
                                   st.bbox_min[1], st.bbox_min[2], st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area);
                        done += std::string(done.empty() ? "" : " ") + (c.name + 1) + " " + std::to_string(c.radius);
                        continue;
                    }
                    plainSteps = true;
                    const int rc = c.op == -1 ? canvas.DetachRegion(cleanElement, c.radius, &st)
                                 : c.op == 0 ? canvas.FillRegionHoles(6, &st)
                                             : canvas.MorphRegion(c.op, cleanElement, c.radius, &st);
                    if (rc != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                    done += std::string(done.empty() ? "" : " ") + (c.name + 1);
                    if (c.op != 0) done += " " + std::to_string(c.radius);
                }
                if (svr_region_measure(&st, sp, &m) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                if (!plainSteps)
                    ;                                              // (-largest / -minsize alone: their own lines say it all)
                else if (st.status == SVR_REGION_STATUS_EMPTY)
                    printf("cleaned (%s, element %d): the region is empty\n", done.c_str(), cleanElement);
                else
                    printf("cleaned (%s, element %d): %llu voxels, volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g\n",
                           done.c_str(), cleanElement, (unsigned long long)st.voxels, m.volume, m.mean, m.stddev, st.vmin, st.vmax, st.bbox_min[0], st.bbox_min[1],
                           st.bbox_min[2], st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area);
            }
            if (smoothPartsSize >= 0.0 && !growcut) {                   // the parts of the cleaned region, all at once
                uint32_t parts = 0u;
                if (canvas.LabelRegion(growConn, &parts) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                char what[64];
                snprintf(what, sizeof what, "%u parts conn %d", parts, growConn);
                if (!smoothParts(what)) return 1;
            }
            if (!scissorSteps.empty() || fillBetweenAxis >= 0 || smoothRegionOp || (growcut && !cleanSteps.empty())) partsSmoothed = false;   // (those replace the region)
            for (const ScissorStep& sc : scissorSteps) {                // cut or paint with a closed line on the picture, or on a slice picture
                int rc;
                if (sc.axis < 0) rc = canvas.ScissorRegion(sc.polygon, sc.op, &st);
                else {
                    svr_slice_params sp2;
                    rc = svr_slice_params_axis(&sp2, &canvas.Volume(), sc.axis, sc.pos, (uint32_t)W, (uint32_t)H);
                    if (rc == 0) rc = canvas.ScissorRegionOnSlice(sp2, (uint32_t)W, (uint32_t)H, sc.polygon, sc.op, sc.thickness, &st);
                }
                if (rc == 0) rc = svr_region_measure(&st, sp, &m);
                if (rc != 0) { fprintf(stderr, "-scissor: %s\n", svr_last_error_code() ? svr_last_error() : "not a polygon the scissors take"); return 1; }
                float ms = 0.f;
                svr_region_scissor_last_ms(&ms);
                const char* const what = sc.op == SVR_SCISSOR_ERASE_INSIDE ? "inside" : sc.op == SVR_SCISSOR_ERASE_OUTSIDE ? "outside" : "fill";
                char view[64] = "";
                if (sc.axis >= 0) snprintf(view, sizeof view, "-slice %c %g thickness %g", "xyz"[sc.axis], sc.pos, sc.thickness);
                if (st.status == SVR_REGION_STATUS_EMPTY)
                    printf("scissor%s %s, %zu vertices: the region is empty; %.3f ms\n", view, what, sc.polygon.size() / 2, ms);
                else
                    printf("scissor%s %s, %zu vertices: %llu voxels, volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g; %.3f ms\n", view, what,
                           sc.polygon.size() / 2, (unsigned long long)st.voxels, m.volume, m.mean, m.stddev, st.vmin, st.vmax, st.bbox_min[0], st.bbox_min[1],
                           st.bbox_min[2], st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area, ms);
            }
            if (fillBetweenAxis >= 0) {                                 // the slices between the drawn ones
                svr_fill_between_info fb;
                int rc = canvas.FillRegionBetweenSlices(fillBetweenAxis, &st, &fb);
                if (rc == 0) rc = svr_region_measure(&st, sp, &m);
                if (rc != 0) { fprintf(stderr, "-fill-between: %s\n", svr_last_error()); return 1; }
                float ms = 0.f;
                svr_region_fill_between_last_ms(&ms);
                printf("fill-between %c: %u keys (%d .. %d), %u gaps, %u slices filled, %llu -> %llu voxels", "xyz"[fillBetweenAxis], fb.keys, (int)fb.first_key,
                       (int)fb.last_key, fb.gaps, fb.filled_slices, (unsigned long long)fb.voxels_in, (unsigned long long)fb.voxels_out);
                if (st.status == SVR_REGION_STATUS_EMPTY)
                    printf("; the region is empty; %.3f ms\n", ms);
                else
                    printf(", volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g; %.3f ms\n", m.volume, m.mean, m.stddev, st.vmin, st.vmax,
                           st.bbox_min[0], st.bbox_min[1], st.bbox_min[2], st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area, ms);
            }
            if (smoothRegionOp) {                                       // the ragged boundary
                const uint64_t before = st.voxels;
                int rc = canvas.SmoothRegion(smoothRegionOp, smoothRegionSize, (uint32_t)smoothRegionN, &st);
                if (rc == 0) rc = svr_region_measure(&st, sp, &m);
                if (rc != 0) { fprintf(stderr, "-smooth-region: %s\n", svr_last_error()); return 1; }
                float ms = 0.f;
                svr_region_smooth_last_ms(&ms);
                printf("smooth-region %s %g x %d: %llu -> %llu voxels", smoothRegionOp == SVR_SMOOTH_MAJORITY ? "median" : "gauss", smoothRegionSize, smoothRegionN,
                       (unsigned long long)before, (unsigned long long)st.voxels);
                if (st.status == SVR_REGION_STATUS_EMPTY)
                    printf("; the region is empty; %.3f ms\n", ms);
                else
                    printf(", volume %g, mean %.1f +- %.1f (raw %u..%u), box %d %d %d .. %d %d %d, surface %g; %.3f ms\n", m.volume, m.mean, m.stddev, st.vmin, st.vmax,
                           st.bbox_min[0], st.bbox_min[1], st.bbox_min[2], st.bbox_max[0], st.bbox_max[1], st.bbox_max[2], m.surface_area, ms);
            }
            if (thickness) {
                double radius = 0.0;
                int32_t at[3] = {-1, -1, -1};
                const int rc = canvas.RegionThickness(&radius, at);
                if (rc < 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                if (rc == SVR_REGION_STATUS_EMPTY) printf("largest inscribed ball: none (the region is empty or fills the volume)\n");
                else printf("largest inscribed ball: radius %g at voxel %d %d %d\n", radius, at[0], at[1], at[2]);
            }
            if (!compareMaskFile.empty()) {                             // the final region against a saved mask: overlap and surface distances
                svr_compare_measurement m;
                svr_region_comparison c;
                if (canvas.CompareRegionWithFile(compareMaskFile, &m, &c) != 0) {
                    fprintf(stderr, "-compare-mask %s: %s\n", compareMaskFile.c_str(), svr_last_error_code() ? svr_last_error() : "not a one-byte mask of the volume's dimensions");
                    return 1;
                }
                printf("compare-mask: dice %.17g jaccard %.17g hd %.17g hd95 %.17g assd %.17g mm (both %llu, region only %llu, file only %llu voxels)\n", m.dice,
                       m.jaccard, m.hausdorff, m.hausdorff_q, m.assd, (unsigned long long)c.overlap[SVR_OVERLAP_BOTH],
                       (unsigned long long)c.overlap[SVR_OVERLAP_A_ONLY], (unsigned long long)c.overlap[SVR_OVERLAP_B_ONLY]);
            }
            if (!meshFile.empty() && (canvas.ExtractRegionSurface((uint32_t)(meshRelax < 0 ? 0 : meshRelax)) != 0 || !exportSurface(meshFile))) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
            if (!saveMaskFile.empty()) {
                const auto t0 = std::chrono::steady_clock::now();
                if (canvas.SaveRegion(saveMaskFile) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                saved("save-mask", saveMaskFile, canvas.volumeReader->dim, t0);
            }
            if (!savePartsFile.empty()) {
                const auto t0 = std::chrono::steady_clock::now();
                uint32_t parts = 0u;
                const bool smoothed = canvas.RegionLabels() && partsSmoothed;                                // what -smooth-parts left is still the region's
                const bool classes = canvas.RegionLabels() && growcut && !keepClass && cleanSteps.empty();   // the class map of -growcut is still the region's
                if ((!classes && !smoothed && canvas.LabelRegion(growConn, &parts) != 0) || canvas.SaveRegionParts(savePartsFile) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                if (classes) printf("save-parts: the classes of -growcut\n");
                else if (smoothed) printf("save-parts: the parts of -smooth-parts\n");
                else printf("save-parts conn %d: %u parts\n", growConn, parts);
                saved("save-parts", savePartsFile, canvas.volumeReader->dim, t0);
            }
            if (!saveCropVolume.empty()) {
                const auto t0 = std::chrono::steady_clock::now();
                int32_t d[3] = {0, 0, 0};
                const int rc = canvas.SaveRegionCrop(saveCropVolume, saveCropMask, saveCropMargin, d);
                if (rc < 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                if (rc == SVR_REGION_STATUS_EMPTY) printf("save-crop: the region is empty; nothing is written\n");
                else saved("save-crop", saveCropVolume + " " + saveCropMask, d, t0);
            }
            if (overlay) {
                // the volume is drawn as it was loaded, and the region is laid over the picture
                if (densitySize >= 0.0 && canvas.ShowRegionDensity(densitySize) != 0) { fprintf(stderr, "-density: %s\n", svr_last_error()); return 1; }
                if (overlayParts && !(canvas.RegionLabels() && partsSmoothed)) {
                    uint32_t parts = 0u;
                    if (canvas.LabelRegion(overlayParts, &parts) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                    printf("overlay parts conn %d: %u parts\n", overlayParts, parts);
                }
            }
            else if ((densitySize >= 0.0 ? canvas.ShowRegionDensity(densitySize) : canvas.ShowRegion(growMode, 0u)) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
        }
        if (!meshIsoFile.empty() && (canvas.ExtractIsoSurface((uint32_t)meshIsoLevel, 0u) != 0 || !exportSurface(meshIsoFile))) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
        svr_overlay_style overlayStyle;
        svr_overlay_style_default(&overlayStyle);
        overlayStyle.fill_alpha = (uint32_t)overlayFill; overlayStyle.edge_alpha = (uint32_t)overlayEdge;

        if (sliceAxis >= 0) {
            // one slice (or a stack of them) instead of a rendering
            if (canvas.SetSlice(sliceAxis, slicePos) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
            svr_slice_params sp = canvas.Slice();
            if (slabMode) { sp.thickness = slabThickness; sp.mode = slabMode; sp.step = sqrtf(sp.u.x * sp.u.x + sp.u.y * sp.u.y + sp.u.z * sp.u.z); }
            sp.window_lo = proj.window_lo; sp.window_hi = proj.window_hi;
            sp.flags = (proj.flags & SVR_PROJ_COLOR_TF) ? SVR_SLICE_COLOR_TF : 0u;
            canvas.SetSlice(sp);
            if (stack == 0) {
                canvas.SetRenderMode(RENDER_MODE_SLICE);
                canvas.paintGL();
                if (svr_last_error_code()) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                if (overlay && canvas.OverlayRegionOnSlice(sp, &overlayStyle) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                if (!canvas.SaveImage(out)) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                printf("slice %c at %g on %s -> %s\n", "xyz"[sliceAxis], slicePos, svr_device_info(), out.c_str());
            } else {
                // from POS to the far face along the plane's normal n = normalize(cross(u, v)): -x, +y, -z for the three axes
                svr_slice_params far;
                if (svr_slice_params_axis(&far, &canvas.Volume(), sliceAxis, sliceAxis == 1 ? 1.f : 0.f, (uint32_t)W, (uint32_t)H) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                const float c0 = sliceAxis == 0 ? sp.center.x : sliceAxis == 1 ? sp.center.y : sp.center.z;
                const float c1 = sliceAxis == 0 ? far.center.x : sliceAxis == 1 ? far.center.y : far.center.z;
                const float spacing = stack > 1 ? fabsf(c1 - c0) / (float)(stack - 1) : 0.f;
                const size_t bytes = (size_t)W * H * 4;
                void* imgs = svr_device_malloc(bytes * (size_t)stack);
                if (!imgs) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                int rc = svr_render_slice_stack(imgs, &canvas.Volume(), &canvas.TransferFunctionPod(), (uint32_t)W, (uint32_t)H, &sp, (uint32_t)stack, spacing);
                if (rc == 0 && overlay) {
                    const svr_overlay_source src = {canvas.RegionLabels() ? nullptr : canvas.RegionMask(), canvas.RegionLabels()};
                    const int* dim = canvas.volumeReader->dim;
                    rc = svr_overlay_slice(imgs, &canvas.Volume(), dim[0], dim[1], dim[2], (uint32_t)W, (uint32_t)H, &sp, (uint32_t)stack, spacing, &src, &overlayStyle);
                }
                std::vector<uint8_t> host(bytes);
                const std::string stem = out.size() > 4 && out.compare(out.size() - 4, 4, ".tga") == 0 ? out.substr(0, out.size() - 4) : out;
                for (int k = 0; rc == 0 && k < stack; ++k) {
                    char name[32];
                    snprintf(name, sizeof name, "_%04d.tga", k);
                    if (svr_memcpy_d2h(host.data(), (const uint8_t*)imgs + bytes * (size_t)k, bytes) != 0 ||
                        svr_tga_write((stem + name).c_str(), W, H, host.data()) != 0) break;
                }
                svr_device_free(imgs);
                if (rc != 0 || svr_last_error_code()) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
                printf("%d slices %c from %g, %g apart, on %s -> %s_0000.tga ...\n", stack, "xyz"[sliceAxis], slicePos, spacing, svr_device_info(), stem.c_str());
            }
            svr_shutdown();
            return 0;
        }

        if (adaptiveTarget > 0.f && !raycast) {
            const auto t0 = std::chrono::steady_clock::now();
            svr_adaptive_result r = {};
            const int rc = canvas.PaintAdaptive(adaptiveTarget, 0u, frames > 0 ? (uint32_t)frames : 1u, &r);
            svr_device_synchronize();
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rc != 0 || svr_last_error_code()) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
            printf("adaptive target %g: %u..%u frames per tile in %.1f ms, %llu samples, %u of %u x %u tiles still active; rmse %.5f, largest tile %.5f\n",
                   adaptiveTarget, r.frames_min, r.frames_max, ms, (unsigned long long)r.pixel_frames, r.tiles_active, r.tiles_x, r.tiles_y, r.rmse, r.tile_max);
        } else if (noiseTarget > 0.f && !raycast) {
            const auto t0 = std::chrono::steady_clock::now();
            const uint32_t used = canvas.RenderUntil(noiseTarget, 0.f, frames > 0 ? (uint32_t)frames : 1u);
            svr_device_synchronize();
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            const svr_noise_estimate e = canvas.GetNoiseEstimate();
            if (svr_last_error_code()) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
            printf("noise target %g: %u frames in %.1f ms; estimate at %u frames (against %u): rmse %.5f, largest tile %.5f, %llu pixels, %llu non-finite\n",
                   noiseTarget, used, ms, e.frames, e.frames_ref, e.rmse, e.tile_max, (unsigned long long)e.pixels, (unsigned long long)e.nonfinite);
        } else
            for (int f = 0; f < (raycast ? 1 : frames); ++f) canvas.paintGL();
        if (svr_last_error_code()) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
        if (overlay) {
            // the hit map that belongs to the picture: the ray caster's opacity level, the isosurface point, the MIP sample
            svr_hit_params hp = hitParams;
            if (project) { hp.mode = proj.mode == SVR_PROJ_ISO ? SVR_HIT_ISO : SVR_HIT_MAX; hp.iso = proj.iso; }
            if (canvas.OverlayRegion(hp, &overlayStyle) != 0) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
        }
        if (!canvas.SaveImage(out)) { fprintf(stderr, "%s\n", svr_last_error()); return 1; }
        printf("%u frame(s) on %s -> %s\n", canvas.FrameNo(), svr_device_info(), out.c_str());
    }
    svr_shutdown();
    return 0;
}
