"""Region bookkeeping for the frame stream's reuse (procedure.genFrameStream(reuse=True)): which tiles of which step have to run for a frame, given
the cells of the raw frame that differ from the frame before it.  Integers and numpy only -- no torch, no device.

A REGION is a boolean cell map of an image: cell (i, j) covers the pixels [16 i, 16 i + 16) x [16 j, 16 j + 16) (clipped at the bottom and right edges) and is True where
the image may differ from the previous frame's image at the same point of the chain.  Every rule below keeps the one property the exactness argument needs: a pixel
outside the region is bit-identical to the previous frame's.  For the first step the region is the device's change map itself (moe_changed_blocks), which is exact.

  support of a tile   the pixels of the step's (unpadded) input image the tile reads: its input rectangle in the padded image's coordinates, mapped back -- the part
                      inside the image as it is, rows / columns past the bottom / right edge through padImage's reflection (edge not repeated, up to len - 1 samples;
                      the zeros behind it depend on nothing)
  step rule           a tile runs iff its support touches a True cell; the step's output region is the union of the HR extents [top sc, bsc) x [left sc, rsc) of the
                      tiles that ran, clipped to the output (the fold rewrites the canvas from the pool: outside that union every contributing tile is last frame's).
                      A DN step's blend with its input is pointwise and its input differs only inside the input region, which the run tiles' extents cover
  resize rule         a changed source rectangle reaches the output pixels whose taps can touch it (nearest 1 tap, bilinear 2, bicubic 4, align_corners = False),
                      dilated by one pixel on either side for the rounding of the kernel's float coordinates: a superset
  everything else     a step without a rule (an SR with ensemble > 0) runs whole and marks its whole output; so does a step whose plan object is not the one it used for
                      the previous frame (the first frame, a re-plan, an eviction from the Option's plan cache): Tracker
"""
import numpy as np

CELL = 16
TAPS = {'nearest': 1, 'bilinear': 2, 'bicubic': 4}


def cells(h, w):
    """The cell grid of an h x w image."""
    return -(-int(h) // CELL), -(-int(w) // CELL)


def none(h, w):
    return np.zeros(cells(h, w), dtype=bool)


def full(h, w):
    return np.ones(cells(h, w), dtype=bool)


def markRects(h, w, rects):
    """The region of an h x w image that covers the pixel rectangles (r0, r1, c0, c1), half-open."""
    m = none(h, w)
    for r0, r1, c0, c1 in rects:
        r0, r1, c0, c1 = max(r0, 0), min(r1, h), max(c0, 0), min(c1, w)
        if r1 > r0 and c1 > c0:
            m[r0 // CELL:-(-r1 // CELL), c0 // CELL:-(-c1 // CELL)] = True
    return m


def rectsOf(region):
    """The True cells of a region as pixel rectangles (one per run of cells in a cell row; not clipped to the image)."""
    out = []
    for i in np.flatnonzero(region.any(axis=1)):
        row = np.flatnonzero(region[i])
        cuts = np.flatnonzero(np.diff(row) > 1)
        for a, b in zip(np.concatenate(([0], cuts + 1)), np.concatenate((cuts, [len(row) - 1]))):
            out.append((int(i) * CELL, int(i) * CELL + CELL, int(row[a]) * CELL, int(row[b]) * CELL + CELL))
    return out


def axisSupport(a, b, n, to):
    """The source intervals an interval [a, b) of a padded axis reads: the axis has n samples and is padded to `to` (0 or <= n: not padded) by padImage's rule --
    index i in [n, n + min(n - 1, to - n)) holds sample 2 n - 2 - i, the indices behind hold zeros."""
    out = []
    if min(b, n) > a:
        out.append((a, min(b, n)))
    refl = min(n - 1, max(0, int(to or 0) - n))
    lo, hi = max(a, n), min(b, n + refl)
    if hi > lo:
        out.append((2 * n - 1 - hi, 2 * n - 1 - lo))
    return out


def tileSupport(tile, H, W, padHTo=0, padWTo=0):
    """The support of a tile (top, bottom, left, right, ..) of a plan for an H x W image: pixel rectangles of the unpadded image."""
    top, bottom, left, right = (int(v) for v in tile[:4])
    return [(r0, r1, c0, c1) for r0, r1 in axisSupport(top, bottom, H, padHTo) for c0, c1 in axisSupport(left, right, W, padWTo)]


class PlanRegions(object):
    """What the step rule reads of a plan (imageProcess.TilePlan or anything with its shape, tiles, sc, outH, outW, padHTo, padWTo): per tile the support as cell
    slices of the input image and the HR extent."""

    def __init__(self, plan):
        _, H, W = plan.shape
        self.inHW, self.outHW, self.n_tiles = (int(H), int(W)), (int(plan.outH), int(plan.outW)), len(plan.tiles)
        self.support = [tileSupport(t, H, W, plan.padHTo, plan.padWTo) for t in plan.tiles]
        self.slices = [[(slice(r0 // CELL, -(-r1 // CELL)), slice(c0 // CELL, -(-c1 // CELL))) for r0, r1, c0, c1 in s] for s in self.support]
        sc = int(plan.sc)
        self.extent = [(t[0] * sc, min(t[6], plan.outH), t[2] * sc, min(t[7], plan.outW)) for t in plan.tiles]
        self.pixels = [(t[1] - t[0]) * (t[3] - t[2]) for t in plan.tiles]          # input pixels of one plane of the tile


def runSet(regions, changed):
    """The step rule's first half: uint8 mask over the plan's tiles, 1 = the tile's support touches a changed cell."""
    if tuple(changed.shape) != cells(*regions.inHW):
        raise ValueError('reuse: a region of {} cells for an image of {} x {} ({} cells)'.format(tuple(changed.shape), regions.inHW[1], regions.inHW[0], cells(*regions.inHW)))
    return np.array([1 if any(changed[s].any() for s in sl) else 0 for sl in regions.slices], dtype=np.uint8)


def outRegion(regions, mask):
    """The step rule's second half: the region of the step's output, the union of the HR extents of the tiles that ran."""
    return markRects(regions.outHW[0], regions.outHW[1], [e for e, m in zip(regions.extent, mask) if m])


def resizeAxis(a, b, n, m, mode):
    """The output interval of an axis resized from n to m samples whose taps can touch the source interval [a, b).  The source coordinate of output o is o n / m for
    nearest and ((2 o + 1) n - m) / (2 m) otherwise (align_corners = False); a tap set of T samples around it touches [a, b) only if the coordinate lies in
    [a - T, b + T) -- T = 1, 2, 3 for nearest, bilinear, bicubic: the taps' reach and one sample for the float coordinate's rounding.  Taps past either end clamp to the
    edge sample, which the interval covers when it holds that sample.  One more output pixel on either side."""
    T = {1: 1, 2: 2, 4: 3}[TAPS[mode]]
    A, B = a - T, b + T
    if mode == 'nearest':
        lo, hi = (A * m) // n, -((-B * m) // n)
    else:
        lo, hi = ((2 * A + 1) * m - n) // (2 * n), -((-((2 * B + 1) * m - n)) // (2 * n)) + 1
    lo, hi = lo - 1, hi + 1
    if A <= 0:
        lo = 0
    if B >= n:
        hi = m
    return max(lo, 0), min(hi, m)


def resizeRect(rect, inHW, outHW, mode):
    """The resize rule for one pixel rectangle: (r0, r1, c0, c1) of the inHW image -> the rectangle of the outHW image it can change."""
    r0, r1 = resizeAxis(rect[0], rect[1], inHW[0], outHW[0], mode)
    c0, c1 = resizeAxis(rect[2], rect[3], inHW[1], outHW[1], mode)
    return r0, r1, c0, c1


def resizeRegion(changed, inHW, outHW, mode):
    """The resize rule for a region."""
    if mode not in TAPS:
        raise ValueError('reuse: no resize rule for mode "{}"'.format(mode))
    clip = lambda r: (r[0], min(r[1], inHW[0]), r[2], min(r[3], inHW[1]))
    return markRects(outHW[0], outHW[1], [resizeRect(clip(r), inHW, outHW, mode) for r in rectsOf(changed)])


class Tracker(object):
    """What a stream remembers between frames: per key (a step and an image of the chain) the plan object the step ran with for the previous frame.  step() applies
    the step rule, or the fallback when there is no previous frame under that plan."""

    def __init__(self):
        self.plans, self._regions = {}, {}

    def regions(self, plan):
        ent = self._regions.get(id(plan))
        if ent is None or ent[0] is not plan:
            if len(self._regions) > 16:
                self._regions.clear()
            ent = self._regions[id(plan)] = (plan, PlanRegions(plan))      # (the plan is kept alive beside its id)
        return ent[1]

    def step(self, key, plan, changed, rule=True):
        """-> (mask, region of the output).  changed: the region of the step's input, None = unknown; rule = False: the step has no rule.  Everything runs and the
        whole output is marked unless the plan object is the one `key` ran with last time, the input region is known and the step has a rule."""
        reg = self.regions(plan)
        same = self.plans.get(key) is plan
        self.plans[key] = plan
        if not (same and rule and changed is not None):
            return np.ones(reg.n_tiles, dtype=np.uint8), full(*reg.outHW)
        mask = runSet(reg, changed)
        return mask, outRegion(reg, mask)

    def forget(self, key):
        """The next step() of `key` runs everything (its retained results are gone)."""
        self.plans.pop(key, None)


def walk(tracker, image, steps, changed, hw):
    """A chain without the device: steps as ('tiles', plan[, rule]) | ('resize', (h, w), mode) | ('opaque',), applied to the region `changed` of the chain's input for
    the image `image` of hw = (height, width) (None: unknown) exactly as the stream applies them.  -> (per step the mask of its tiles, None for a step without tiles; the region of the
    chain's output, None = all of it).  What the stream's own walk does step by step while it runs them; here for planning and for the tests."""
    masks, hw = [], tuple(hw)
    for i, step in enumerate(steps):
        if step[0] == 'tiles':
            mask, changed = tracker.step((i, image), step[1], changed, *step[2:3])
            masks.append(mask)
            hw = tracker.regions(step[1]).outHW
            continue
        masks.append(None)
        if step[0] == 'resize':
            if changed is not None:
                changed = resizeRegion(changed, hw, step[1], step[2])
            hw = tuple(step[1])
        else:
            changed = None
    return masks, changed
