"""`-vf thumbnail` restated for the tests: the per-plane histograms by np.bincount, the
filter's selection as plain index loops over C doubles, the frames a segment's groups keep, and the
shapes and contents the kernel is tried on.  Nothing here imports the package's own thumbnail code."""
import numpy as np

CHROMA_SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}

# (w, h, chroma, frames): where k_frame_hist can go wrong
GPU_SHAPES = [
    (3, 3, "444", 3),       # byte path only
    (16, 16, "420", 3),     # chroma below one piece
    (33, 17, "444", 4),     # odd frame bytes: frames 1.. are misaligned
    (130, 66, "422", 3),    # a 4:2:2 source, 65 x 66 chroma planes of odd width
    (4100, 5, "420", 2),    # a plane of more than one workgroup, with a byte tail
    (640, 360, "420", 3),   # several workgroups per plane and frame
]
CONTENTS = ("noise", "constant", "checker")


def plane_sizes(w, h, c):
    hs, vs = CHROMA_SHIFTS[c]
    cn = ((w + hs) >> hs) * ((h + vs) >> vs)
    return [w * h, cn, cn]


def frame_bytes(w, h, c):
    return sum(plane_sizes(w, h, c))


HIST_WG_BYTES = 256 * 4 * 16   # scale.hip: kHistThreads threads, kHistVecs 16-byte pieces each: 16 KiB of one plane


def hist_gpf(w, h, c):
    """hist_plan's workgroups per frame: ceil(bytes / 16 KiB) for Y, then for U, then for V.  A call of n frames
    launches gpf n workgroups in x, t = 0 .. gpf n - 1, the frame of each by a multiply-high division."""
    return sum((nb + HIST_WG_BYTES - 1) // HIST_WG_BYTES for nb in plane_sizes(w, h, c))


def make_frames(kind, w, h, c, n, seed=0):
    """(n, frame_bytes) uint8: every plane of every frame different, so a plane or frame mix-up shows.
    noise: uniform bytes, every value put in where the plane has room for all 256; constant: one value a
    plane; checker: two values a plane, alternating sample by sample."""
    rng = np.random.default_rng([seed, w, h, n])
    out = np.empty((n, frame_bytes(w, h, c)), np.uint8)
    for f in range(n):
        at = 0
        for p, nb in enumerate(plane_sizes(w, h, c)):
            if kind == "noise":
                v = rng.integers(0, 256, nb, dtype=np.uint8)
                if nb >= 256:
                    v[rng.permutation(nb)[:256]] = np.arange(256, dtype=np.uint8)
            elif kind == "constant":
                v = np.full(nb, (37 + 71 * p + 13 * f) & 255, np.uint8)
            else:
                a, b = (16 + 40 * p + 3 * f) & 255, (235 - 50 * p - 7 * f) & 255
                v = np.where(np.arange(nb) & 1, b, a).astype(np.uint8)
            out[f, at:at + nb] = v
            at += nb
    return out


def hist_ref(frames, w, h, c):
    """(n, 768) uint32: hist[f][256 p + v] = samples of value v in plane p of frame f."""
    frames = np.asarray(frames, np.uint8).reshape(-1, frame_bytes(w, h, c))
    out = np.zeros((len(frames), 768), np.uint32)
    for f, fr in enumerate(frames):
        at = 0
        for p, nb in enumerate(plane_sizes(w, h, c)):
            out[f, 256 * p:256 * p + 256] = np.bincount(fr[at:at + nb], minlength=256)
            at += nb
    return out


def pick_ref(hists):
    """The filter's loops, index by index, on np.float64 scalars (C doubles)."""
    h = np.asarray(hists)
    n = h.shape[0]
    avg = np.zeros(768, np.float64)
    for j in range(768):
        for i in range(n):
            avg[j] = avg[j] + np.float64(h[i][j])
        avg[j] = avg[j] / np.float64(n)
    best, best_e = -1, np.float64(0)
    for i in range(n):
        e = np.float64(0)
        for j in range(768):
            d = avg[j] - np.float64(h[i][j])
            e = e + d * d
        if i == 0 or e < best_e:
            best, best_e = i, e
    return best


def kept_frames(hists, step, N):
    """The segment's frame indices that `framestep=step,thumbnail=N` hands on, for the (nframes, 768)
    histograms of all its frames: frames 0, step, 2 step, ... in groups of N, the last group the remainder."""
    kept = list(range(0, len(hists), step))
    return [kept[g + pick_ref([hists[k] for k in kept[g:g + N]])] for g in range(0, len(kept), N)]
