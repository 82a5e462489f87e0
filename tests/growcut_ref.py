"""Test-side reference of the grow-from-seeds calls (include/svr_abi.h, "grow from seeds"), numpy only and literal: the Jacobi iteration
of tests/geodesic_ref.py on packed keys (cost << 32) | zone with the image term in the cost of a move and an add that saturates at CAP, an
independent heap Dijkstra with the same saturation, a sequential Gauss-Seidel in a given voxel order, and the two marker calls.  Nothing
here knows about tiles, sweeps or dirty maps."""
import heapq

import numpy as np

from tests import geodesic_ref as gr

NONE = gr.NONE
CAP = 0xFFFFFFFE
KEY_NONE = gr.KEY_NONE
MAX_MOVE = 0x7FFFFFFF
_S32 = np.uint64(32)
_LOW = np.uint64(0xFFFFFFFF)


def default_weights(connectivity):
    """The step weights of svr_region_growcut_params_default."""
    return tuple(1 if c < gr.CLASSES[connectivity] else 0 for c in range(7))


def refused(weights, gain, shift):
    """The parameter refusals of the contract."""
    return not any(weights) or gain > 65535 or shift > 15 or max(int(w) for w in weights) + gain * (65535 >> shift) > MAX_MOVE


def shifted(a, off, fill):
    """b[p] = a[p - off], `fill` where p - off lies outside."""
    out = np.full_like(a, fill)
    src, dst = [], []
    for o, n in zip(off, a.shape):
        if abs(o) >= n:
            return out
        src.append(slice(max(0, -o), n - max(0, o)))
        dst.append(slice(max(0, o), n - max(0, -o)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def split_keys(key):
    cost = (key >> _S32).astype(np.uint32)
    zones = np.where(cost != NONE, key & _LOW, 0).astype(np.uint32)
    return cost, zones


def start_keys(labels, domain):
    return np.where(domain & (labels != 0), labels.astype(np.uint64), KEY_NONE)


def growcut(vox, labels, domain=None, weights=default_weights(26), gain=1, shift=0):
    """(cost, zones) as uint32 arrays [nz][ny][nx]; domain None = the whole volume."""
    vox = np.asarray(vox, dtype=np.uint16)
    labels = np.asarray(labels, dtype=np.uint32)
    domain = np.ones(vox.shape, dtype=bool) if domain is None else np.asarray(domain, dtype=bool)
    assert not refused(weights, gain, shift)
    img = vox.astype(np.int64)
    key = start_keys(labels, domain)
    mv = gr.moves(weights)
    while True:
        new = key.copy()
        for off, w in mv:
            s = shifted(key, off, KEY_NONE)
            move = (w + gain * (np.abs(img - shifted(img, off, 0)) >> shift)).astype(np.uint64)
            total = np.minimum((s >> _S32) + move, np.uint64(CAP))                        # the saturating add
            cand = np.where((s >> _S32) != np.uint64(NONE), (total << _S32) | (s & _LOW), KEY_NONE)
            np.minimum(new, cand, out=new)
        new[~domain] = KEY_NONE
        if np.array_equal(new, key):
            break
        key = new
    return split_keys(key)


def move_cost(img, p, q, w, gain, shift):
    return w + gain * (abs(int(img[p]) - int(img[q])) >> shift)


def dijkstra(vox, labels, domain=None, weights=default_weights(26), gain=1, shift=0):
    """The same pair by an independent method: a heap that pops (cost, label, voxel); an extension saturates at CAP."""
    vox = np.asarray(vox, dtype=np.uint16)
    domain = np.ones(vox.shape, dtype=bool) if domain is None else np.asarray(domain, dtype=bool)
    nz, ny, nx = domain.shape
    cost = np.full(domain.shape, NONE, dtype=np.uint32)
    zones = np.zeros(domain.shape, dtype=np.uint32)
    done = np.zeros(domain.shape, dtype=bool)
    heap = [(0, int(labels[p]), p) for p in map(tuple, np.argwhere(domain & (labels != 0)).tolist())]
    heapq.heapify(heap)
    mv = gr.moves(weights)
    while heap:
        d, lab, p = heapq.heappop(heap)
        if done[p]:
            continue
        done[p], cost[p], zones[p] = True, d, lab
        for (dz, dy, dx), w in mv:
            q = (p[0] + dz, p[1] + dy, p[2] + dx)
            if 0 <= q[0] < nz and 0 <= q[1] < ny and 0 <= q[2] < nx and domain[q] and not done[q]:
                heapq.heappush(heap, (min(d + move_cost(vox, p, q, w, gain, shift), CAP), lab, q))
    return cost, zones


def gauss_seidel(vox, labels, domain, weights, gain, shift, order):
    """Chaotic relaxation as the device does it, one voxel at a time in the order `order` (a list of (z, y, x)), repeated until a
    whole pass lowers nothing; python integers."""
    vox = np.asarray(vox, dtype=np.uint16)
    domain = np.ones(vox.shape, dtype=bool) if domain is None else np.asarray(domain, dtype=bool)
    nz, ny, nx = domain.shape
    none = int(KEY_NONE)
    key = {p: none for p in order}
    for p in order:
        if domain[p] and labels[p]:
            key[p] = int(labels[p])
    mv = gr.moves(weights)
    changed = True
    while changed:
        changed = False
        for p in order:
            if not domain[p]:
                continue
            best = key[p]
            for (dz, dy, dx), w in mv:
                q = (p[0] - dz, p[1] - dy, p[2] - dx)
                if not (0 <= q[0] < nz and 0 <= q[1] < ny and 0 <= q[2] < nx) or (key[q] >> 32) == NONE:
                    continue
                cand = (min((key[q] >> 32) + move_cost(vox, q, p, w, gain, shift), CAP) << 32) | (key[q] & 0xFFFFFFFF)
                best = min(best, cand)
            if best < key[p]:
                key[p], changed = best, True
    out = np.empty(domain.shape, dtype=np.uint64)
    for p, k in key.items():
        out[p] = k
    return split_keys(out)


def seed_classes(seeds, classes, shape):
    """classes[i] on the voxel (x, y, z) of seed i; the lowest i of several on one voxel."""
    out = np.zeros(shape, dtype=np.uint32)
    for (x, y, z), c in reversed(list(zip(seeds, classes))):
        out[z, y, x] = c
    return out


def label_paint(labels, mask, label, only_unlabelled):
    out = np.array(labels, dtype=np.uint32)
    out[mask & (out == 0) if only_unlabelled else mask] = label
    return out


# ---------------------------------------------------------------------------------------------- fixtures shared by the CPU and GPU tests
TILED_SHAPES = [(10, 11, 37), (17, 19, 70)]              # [nz][ny][nx]: two partial tiles per axis; three tiles in x and y
ONE_TILE = (8, 8, 32)
WEIGHT_SETS = {"6": default_weights(6), "18": default_weights(18), "26": default_weights(26), "anisotropic": (2, 3, 5, 4, 6, 7, 9)}
GAINS = [(0, 0), (1, 0), (7, 3), (65535, 15)]            # (contrast_gain, contrast_shift)
DOMAINS = gr.DENSITIES + (None,)                         # a density of the random domain mask, or the NULL domain
VALUES = ("small", "full")                               # voxels from {0 .. 3}: equal-cost paths abound; from the whole u16 range


def random_volume(shape, kind, seed=11):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4 if kind == "small" else 65536, shape, dtype=np.uint16)


def class_markers(shape, n, seed, classes=3):
    """n marker voxels with classes 1 .. `classes`."""
    rng = np.random.default_rng(seed)
    labels = np.zeros(shape, dtype=np.uint32)
    at = rng.choice(labels.size, min(n, labels.size), replace=False)
    labels.reshape(-1)[at] = rng.integers(1, classes + 1, len(at)).astype(np.uint32)
    return labels


def case(shape, kind, density):
    """(vox, labels, domain or None) of a random case."""
    k = DOMAINS.index(density)
    n = int(np.prod(shape))
    domain = None if density is None else gr.random_domain(shape, density, 21 + k)
    return random_volume(shape, kind), class_markers(shape, max(2, min(24, n // 150)), 31 + k), domain


def all_combinations(shape):
    """Every (kind, density, weight set name, (gain, shift)) for a shape small enough to afford the whole product."""
    return [(kind, density, name, gs) for kind in VALUES for density in DOMAINS for name in WEIGHT_SETS for gs in GAINS]


def covering_combinations():
    """For the larger shape: every (kind, density) pair once, and with them every weight set and every (gain, shift) at least once --
    and each weight set with a non-zero gain."""
    names, out = list(WEIGHT_SETS), []
    for i, (kind, density) in enumerate((kind, density) for kind in VALUES for density in DOMAINS):
        out.append((kind, density, names[i % 4], GAINS[(i + 1) % 4 if i < 4 else (i + 2) % 4]))
    out += [("small", 0.7, "26", (1, 0)), ("full", None, "anisotropic", (7, 3))]
    return out


def combinations(shape):
    return covering_combinations() if tuple(shape) == TILED_SHAPES[1] else all_combinations(shape)


def cached_case(shape, kind, density, name, gs):
    vox, labels, domain = case(shape, kind, density)
    return gr.cached(("growcut", tuple(shape), kind, density, name, gs), lambda: growcut(vox, labels, domain, WEIGHT_SETS[name], *gs))


SAT_SHAPE = (1, 1, 40)
SAT_GAIN = 32768


def saturating_line(swapped=False):
    """A line of alternating 0 / 65535 with a seed of label 7 at one end and 3 at the other (the other way round when swapped): under
    gain 32768 a move costs 1 + 32768 * 65535 = 2147450881, so the third move from a seed saturates."""
    vox = np.zeros(SAT_SHAPE, dtype=np.uint16)
    vox[0, 0, 1::2] = 65535
    labels = np.zeros(SAT_SHAPE, dtype=np.uint32)
    labels[0, 0, 0], labels[0, 0, -1] = (3, 7) if swapped else (7, 3)
    return vox, labels


HEAD_N = 48
HEAD_CLASSES = {"brain": 1, "bone": 2, "air": 3}
HEAD_R2 = 4                                              # strokes are balls of radius 2


def head_seeds(vox):
    """[(x, y, z, class)] of two strokes in brain, two in bone and one in air of make_ct_head_volume(48): the bone seeds are the
    brightest voxels of the central row on either side."""
    n = vox.shape[0]
    c = n // 2
    row = vox[c, c, :].astype(np.int64)
    left, right = int(np.argmax(row[:c])), c + int(np.argmax(row[c:]))
    return [(c + 8, c, c, 1), (c - 8, c + 2, c - 3, 1), (left, c, c, 2), (right, c, c, 2), (2, 2, 2, 3)]
