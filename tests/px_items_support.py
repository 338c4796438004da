"""A host model of how the learner's persistent PX16 kernels split a batch into work items (csrc/tron_conv_ws_train.hip,
csrc/tron_conv_ws_kernel.hpp), for tests/test_px_items_model_cpu.py and tests/test_gpu_px_items.py: the geometry tables restated
once, line-for-line models of the launchers, the smallest batch at which every workgroup is in its steady state (a second item
in the other LDS buffer, a third in the first one again, a ragged last round), and which image is which workgroup's k-th item.
Nothing here needs a GPU at import."""
from collections import namedtuple

SIDES = (12, 26, 34)
CHANNELS = ((32, 32), (32, 64), (64, 64))                            # (cin, cout) of the trunk's 3x3 layers
SHAPES = tuple((s, ci, co) for s in SIDES for ci, co in CHANNELS)

# ---- the geometry tables, keyed (side, cin, cout) of the FORWARD layer ------------------------------------------------------
# the weight gradient: dispatch_wgrad_px, csrc/tron_conv_ws_train.hip:459-469 — WCfg<S, NI, R, CO, CI, COT, CIT, KG>
WGRAD_CFG = {
    (12, 64, 64): dict(NI=2, R=8, COT=64, CIT=64, KG=1),
    (12, 32, 64): dict(NI=2, R=8, COT=64, CIT=32, KG=2),
    (12, 32, 32): dict(NI=2, R=8, COT=32, CIT=32, KG=4),
    (26, 64, 64): dict(NI=1, R=6, COT=64, CIT=32, KG=2),
    (26, 32, 64): dict(NI=1, R=6, COT=64, CIT=32, KG=2),
    (26, 32, 32): dict(NI=1, R=6, COT=32, CIT=32, KG=4),
    (34, 64, 64): dict(NI=1, R=5, COT=32, CIT=32, KG=4),
    (34, 32, 64): dict(NI=1, R=5, COT=32, CIT=32, KG=4),
    (34, 32, 32): dict(NI=1, R=5, COT=32, CIT=32, KG=4),
}
# the backward convolution: tron_conv3x3_ws_dgrad, csrc/tron_conv_ws_train.hip:890-898 — TRON_WSB_CASE(S, R, CI, CO, IPI, WAVES)
# with CI = the forward layer's cout and CO = its cin (the backward convolution runs the other way)
WSB_CFG = {
    (12, 32, 32): dict(R=12, IPI=2),
    (12, 32, 64): dict(R=12, IPI=1),
    (12, 64, 64): dict(R=12, IPI=1),
    (26, 32, 32): dict(R=13, IPI=1),
    (26, 32, 64): dict(R=7, IPI=1),
    (26, 64, 64): dict(R=7, IPI=1),
    (34, 32, 32): dict(R=12, IPI=1),
    (34, 32, 64): dict(R=5, IPI=1),
    (34, 64, 64): dict(R=5, IPI=1),
}
# the training forward: TRON_WST_CASES, csrc/tron_conv_ws_train.hip:750-758 — TRON_WST_CASE(S, R, CI, CO, IPI, WAVES, ...)
WST_CFG = {
    (12, 32, 32): dict(R=12, IPI=2),
    (12, 32, 64): dict(R=12, IPI=1),
    (12, 64, 64): dict(R=12, IPI=1),
    (26, 32, 32): dict(R=13, IPI=1),
    (26, 32, 64): dict(R=13, IPI=1),
    (26, 64, 64): dict(R=7, IPI=1),
    (34, 32, 32): dict(R=12, IPI=1),
    (34, 32, 64): dict(R=12, IPI=1),
    (34, 64, 64): dict(R=5, IPI=1),
}
GOUT_GROUPS = 1024                                                   # tron_px16_grad_from_f32: groups = min(batch, 1024), one image at a time


class WgradPlan(namedtuple("WgradPlan", "side cin cout B cus NI R NB KG kinds slabs nwg used parts nstack bytes")):
    """launch_wgrad_px's split: workgroup wb of band b takes stacks wb, wb + nwg[b], ... < nstack, alternating LDS buffers."""

    def items(self, band):
        """The most and the fewest items a workgroup of this band gets."""
        n = self.nwg[band]
        return -(-self.nstack // n), self.nstack // n

    def conditions(self):
        return {
            "two items everywhere": all(self.nstack >= 2 * n for n in self.nwg),
            "three items somewhere": any(self.nstack > 2 * n for n in self.nwg),
            "ragged last round": any(self.nstack % n for n in self.nwg),
            "odd batch at two images per item": self.NI == 1 or self.B % 2 == 1,
        }

    def band_rows(self, band):
        """The stack rows [first, last] of a band (a stack = NI images one under the other, rows 0 .. NI * side - 1)."""
        return band * self.R, min((band + 1) * self.R, self.NI * self.side) - 1

    def locate(self, image, y):
        """(band, workgroup of the band, item index of that workgroup) that reads row y of an image."""
        stack, t = image // self.NI, (image % self.NI) * self.side + y
        band = t // self.R
        return band, stack % self.nwg[band], stack // self.nwg[band]


def wgrad_px_plan(side, cin, cout, B, cus):
    """launch_wgrad_px (csrc/tron_conv_ws_train.hip:412-453), line for line."""
    c = WGRAD_CFG[(side, cin, cout)]
    NI, R, KG = c["NI"], c["R"], c["KG"]
    rows = NI * side
    NB = (rows + R - 1) // R
    assert NB <= 8
    kinds = (cout // c["COT"]) * (cin // c["CIT"])
    per_kind = max(cus // kinds, NB)
    slabs = []
    for b in range(NB):
        r0 = b * R
        nr = min(rows - r0, R)
        slabs.append((nr * side + 31) // 32)
    tot = sum(slabs)
    nstack = (B + NI - 1) // NI
    nwg = [min(max(per_kind * s // tot, 1), nstack) for s in slabs]
    used = sum(nwg)
    parts = used * KG
    return WgradPlan(side, cin, cout, B, cus, NI, R, NB, KG, kinds, tuple(slabs), tuple(nwg), used, parts, nstack, parts * 9 * cout * cin * 4)


class WsPlan(namedtuple("WsPlan", "side cin cout B cus R IPI NB nitems grid")):
    """launch_ws's split: workgroup w takes items w, w + grid, ... < nitems; item i = band i % NB of images (i // NB) * IPI ...."""

    def conditions(self):
        return {
            "two items everywhere": self.nitems >= 2 * self.grid,
            "three items somewhere": self.nitems > 2 * self.grid,
            "ragged last round": self.nitems % self.grid != 0,
            "odd batch at two images per item": self.IPI == 1 or self.B % 2 == 1,
        }

    def items(self):
        """The most and the fewest items a workgroup gets."""
        return -(-self.nitems // self.grid), self.nitems // self.grid

    def images(self, item):
        """The images of an item (the last pair may hold one)."""
        first = item // self.NB * self.IPI
        return [i for i in range(first, first + self.IPI) if i < self.B]

    def item_index(self, image, band=0):
        """(workgroup, its item index) that computes a band of an image."""
        item = image // self.IPI * self.NB + band
        return item % self.grid, item // self.grid


def _ws_plan(table, side, cin, cout, B, cus):
    """launch_ws (csrc/tron_conv_ws_kernel.hpp:832-835)."""
    c = table[(side, cin, cout)]
    R, IPI = c["R"], c["IPI"]
    NB = (side + R - 1) // R
    nitems = (B + IPI - 1) // IPI * NB
    grid = cus // NB * NB
    if nitems < grid:
        grid = nitems
    return WsPlan(side, cin, cout, B, cus, R, IPI, NB, nitems, grid)


def ws_bwd_plan(side, cin, cout, B, cus):
    """tron_conv3x3_ws_dgrad's grid: cin / cout are the forward layer's."""
    return _ws_plan(WSB_CFG, side, cin, cout, B, cus)


def ws_fwd_plan(side, cin, cout, B, cus):
    """tron_conv3x3_ws_train_fwd's grid."""
    return _ws_plan(WST_CFG, side, cin, cout, B, cus)


def steady_batch(plan_fn, side, cin, cout, cus, limit=1 << 16):
    """The smallest batch at which every condition of the plan holds."""
    for B in range(1, limit):
        if all(plan_fn(side, cin, cout, B, cus).conditions().values()):
            return B
    raise AssertionError(f"no steady batch below {limit} for {(side, cin, cout, cus)}")


def tensor_bytes(side, cin, cout, B):
    """The larger of the two f32 tensors of a test at this batch."""
    return B * max(cin, cout) * side * side * 4


# ---- one-hot cases of the weight gradient ---------------------------------------------------------------------------------

OneHot = namedtuple("OneHot", "name image y x ky kx band wb item")


def _pixel(plan, band, il, edge):
    """A gradient pixel (y, x) of image il of a stack inside a band, and a tap (ky, kx) whose input pixel lies inside the image:
    edge 0 = the band's first row of that image at the left border, the tap looking up across the band edge where it can;
    edge 1 = the band's last row of that image at the right border, the tap looking down across the band edge where it can."""
    S = plan.side
    first, last = plan.band_rows(band)
    lo, hi = max(first, il * S) - il * S, min(last, il * S + S - 1) - il * S
    assert 0 <= lo <= hi < S
    if edge == 0:
        y, x = lo, 0
        ky, kx = (0 if y > 0 else 1), 1
    else:
        y, x = hi, S - 1
        ky, kx = (2 if y < S - 1 else 1), 0
    return y, x, ky, kx


def wgrad_one_hot_cases(plan):
    """The images of a steady plan whose stack is, for the workgroup that reads it: the first item, the second (the other buffer),
    the third (the first buffer again), the last stack of a ragged round — and at two images per stack the last stack's only image,
    once more in the band that also holds the missing image's rows, and the second image of a pair right under the separator."""
    assert all(plan.conditions().values())
    NI, S = plan.NI, plan.side
    b3 = min(b for b in range(plan.NB) if plan.nstack > 2 * plan.nwg[b])
    br = max(b for b in range(plan.NB) if plan.nstack % plan.nwg[b])
    b2 = plan.NB // 2
    n1, n2, n3 = plan.nwg[0], plan.nwg[b2], plan.nwg[b3]             # (the last workgroup of band 0, of a middle band; the first of a band with three items)
    picks = [("first item", 0, n1 - 1, 0, 0), ("second item", b2, 2 * n2 - 1, 1, 1), ("third item", b3, 2 * n3, 2, 0),
             ("last stack of the ragged round", br, plan.nstack - 1, (plan.nstack - 1) // plan.nwg[br], 1)]
    cases = []
    for name, band, stack, item, edge in picks:
        first, last = plan.band_rows(band)
        ils = [il for il in range(NI) if il * S <= last and first <= il * S + S - 1 and stack * NI + il < plan.B]
        if not ils:                                                  # (the band lies in the image the last stack does not have)
            band = 0
            ils, item = [0], stack // plan.nwg[0]
        il = ils[-1] if edge == 0 else ils[0]
        y, x, ky, kx = _pixel(plan, band, il, edge)
        cases.append(OneHot(name, stack * NI + il, y, x, ky, kx, band, stack % plan.nwg[band], item))
    if NI == 2:
        # the last stack's only image, its last row: the band below it holds nothing but the rows of the image that is not there
        band = (S - 1) // plan.R
        stack = plan.nstack - 1
        cases.append(OneHot("single-image last stack", plan.B - 1, S - 1, 0, 1, 2, band, stack % plan.nwg[band], stack // plan.nwg[band]))
        # row 0 of a second image: the separator row lies between it and the first image's last row
        band = S // plan.R
        stack = plan.nwg[band] + 1
        cases.append(OneHot("under the stack separator", stack * NI + 1, 0, S - 1, 1, 0, band, 1, 1))
    for c in cases:
        assert 0 <= c.image < plan.B and plan.locate(c.image, c.y) == (c.band, c.wb, c.item), c
        assert 0 <= c.y + c.ky - 1 < S and 0 <= c.x + c.kx - 1 < S, c
    return cases


# ---- planted cases of the backward convolution ----------------------------------------------------------------------------

def ws_planted_images(plan):
    """Of a steady plan: an image every band of which is its workgroup's LAST item, an image every band of which is the FIRST item
    of a workgroup that goes on to three, and the images of the second and third items of one workgroup."""
    assert all(plan.conditions().values())
    NB, grid, nitems = plan.NB, plan.grid, plan.nitems
    k_last = (nitems - 1) // grid                                    # workgroup 0's last item index; nitems and grid are multiples of NB,
    last = plan.images(k_last * grid)[-1]                            # so items k_last * grid .. + NB - 1 exist and are last items too
    w = (nitems - 2 * grid - 1) // NB * NB                           # the last band-0 workgroup that has a third item
    first = plan.images(w)[-1]                                       # (workgroups w .. w + NB - 1 all go on to a second and a third item)
    sums = plan.images(w + grid) + plan.images(w + 2 * grid)
    for b in range(NB):
        wl, kl = plan.item_index(last, b)
        assert kl == k_last >= 2 and wl + (kl + 1) * grid >= nitems
        wf, kf = plan.item_index(first, b)
        assert kf == 0 and wf + 2 * grid < nitems
    assert {plan.item_index(i) for i in sums} == {(w, 1), (w, 2)}
    return {"last": last, "first": first, "sums": sums}
