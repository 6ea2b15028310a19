"""Cases and helpers of the filtered (anti-aliased) views' tests
(test_resample_aa_cpu.py, test_resample_aa_gpu.py): the views of
resample_cases' frame models whose seams are known, the seam count of a view
from its tables, and the <= 2 tiles condition restated from the rule's text
(include/gsvc_amd.h gsvc_render_frames_filtered)."""
import numpy as np
import torch

import resample_cases as RC

# (case, size, crop, aa, seam rows, seam columns): the views of the fused
# against two-pass check.  A seam row is an output row whose ky sub-sample rows
# lie on two source tiles; the counts come from the rule on the CPU and every
# test asserts them from the tables first.
FUSED = [
    ("edge", (12, 17), None, (3, 3), 2, 2),    # four 4-part corner pixels; groups of 9 lanes, 7 pixels a trip
    ("edge", (5, 7), None, (8, 8), 2, 3),  # seams; one pixel per trip
    ("edge", (37, 13), None, (1, 4), 0, 2),   # anisotropic: column seams only
    ("edge", (9, 53), None, (4, 1), 1, 0),    # anisotropic: row seams only
    ("piled", (16, 16), None, (4, 4), 0, 0),     # aligned
    ("piled", (5, 5), None, (8, 8), 3, 3),       # pixel 1 straddles the pile: tiles past 256 and 1024 entries
    ("batch", (7, 11), None, (5, 5), 4, 6),      # three frames, one M = 0; 25 of 64 lanes
    ("batch", (6, 10), (10.25, 3.5, 90.5, 44.0), (4, 4), 1, 5),  # fractional window
    ("wide", (100, 100), None, (3, 3), 12, 12),  # over 256 tiles
    ("wide", (64, 64), None, (4, 4), 0, 0),      # aligned
]
FUSED_IDS = [f"{c}-{s[0]}x{s[1]}-aa{a[0]}x{a[1]}" + ("-crop" if cr else "") for c, s, cr, a, _, _ in FUSED]


def seams(view):
    """(seam rows, seam columns) of a view with ``aa``, from its fine view's
    start tables alone: the output rows (columns) whose sub-samples are not all
    in one tile's range."""
    out = []
    for start, k, n in ((view.fine.row_start, view.aa[0], view.out_h),
                        (view.fine.col_start, view.aa[1], view.out_w)):
        start = np.asarray(start, dtype=np.int64)
        first = np.arange(n) * k
        tile = lambda r: np.searchsorted(start[1:], r, side="right")
        out.append(int((tile(first) != tile(first + k - 1)).sum()))
    return tuple(out)


def two_tiles_ok(src, out, start, extent, k):
    """One axis of the <= 2 tiles condition, from the rule's text: the fine view
    has k * out samples over the same window; the k sub-samples of every output
    pixel lie on the tile of the first one or on the next."""
    _, p, _ = RC.axis(src, k * out, start, extent)
    t = p >> 4
    return all(t[k * i + k - 1] - t[k * i] <= 1 for i in range(out))


def tiny_splats():
    """A 64 x 64 frame of 400 splats about 0.6 px wide on a jittered grid: far
    below a 16 x 16 view's pixel (4 source pixels)."""
    gen = torch.Generator().manual_seed(31)
    H = W = 64
    g = (torch.arange(20, dtype=torch.float32) + 0.5) * (W / 20.0)
    cx, cy = torch.meshgrid(g, g, indexing="xy")
    c = torch.stack([cx.reshape(-1), cy.reshape(-1)], 1) + 2.4 * (torch.rand(400, 2, generator=gen) - 0.5)
    means = (c / torch.tensor([0.5 * W, 0.5 * H]) - 1.0).clamp(-0.99, 0.99)  # pixel = 0.5 (x + 1) W
    chol = torch.tensor([0.6, 0.0, 0.6]).repeat(400, 1) - torch.tensor(RC.BOUND)
    col = 0.3 + 0.7 * torch.rand(400, 3, generator=gen)
    return dict(name="tiny", H=H, W=W, sizes=[400], means=means.contiguous(), chol=chol.contiguous(),
                col=col.contiguous(), bg=torch.zeros(3))
