"""Case table of tests/test_gpu_bn_routes.py: the stand-alone BatchNorm passes (ali_bn_stats, ali_bn_apply, ali_bn_bwd,
ali_bn_stats_from_partials, ali_bn_bwd_from_partials), ali_colsum and ali_act_bwd of csrc/elementwise.hip, one case per
launch route, and a plain restatement of the launch plan (``ew_plan`` there, ``ops.ew_plan`` here) to hold the query to.

Row cases are (B, rows_per_img, C): each is the smallest shape that still takes the route its comment names."""

EW_BLOCK = 256              # kEwBlock: threads of every block
REDUCE_CAP = 512            # reduce_blocks / reduce_blocks_vec cap the reduction grid here
EW_GRID_CAP = 2048          # ew_grid caps the element-wise grid here
EW_CAP = EW_GRID_CAP * EW_BLOCK   # elements (float4 lanes for the vec kernels) one pass of a capped grid covers


def _ceil(a, b):
    return -(-a // b)


def lanes_r(C, vec):
    """row lanes of a reduction block: 256 // (C/4) for the float4 kernels, 256 // pow2ceil(min(C, 256)) otherwise"""
    if vec:
        return EW_BLOCK // (C // 4)
    lc = 1
    while lc < min(C, EW_BLOCK):
        lc <<= 1
    return EW_BLOCK // lc


def raw_reduce_blocks(rows, C, vec):
    """reduction blocks before the cap"""
    return max(1, _ceil(rows, 8 * lanes_r(C, vec)))


def raw_ew_blocks(n, vec):
    """element-wise blocks before the cap (n elements; the vec kernels count float4 lanes)"""
    return max(1, _ceil(n // 4 if vec else n, EW_BLOCK))


def vec_ok(rows, C):
    return C % 4 == 0 and 4 <= C <= 4 * EW_BLOCK and rows * C < 2 ** 31


def plan(op, rows, rows_per_img, C, ld=None, groups=1, aligned=True):
    """what ops.ew_plan must answer, restated from the formulas of include/ali_hip.h / elementwise.hip"""
    ld = C if ld is None else ld
    if (op in ("bn_stats", "bn_bwd") and C > EW_BLOCK) or (op == "colsum" and ld < C):
        return None
    if op == "act_bwd":
        return "scalar", 0, min(EW_GRID_CAP, raw_ew_blocks(rows, False))
    vec = vec_ok(rows * groups, C) and aligned
    if op == "colsum":
        vec = vec and ld % 4 == 0 and rows * ld < 2 ** 31
    nb = min(REDUCE_CAP, raw_reduce_blocks(rows, C, vec)) if op in ("bn_stats", "bn_bwd", "colsum") else 0
    ew = min(EW_GRID_CAP, raw_ew_blocks(rows * C, vec)) if op in ("bn_apply", "bn_bwd", "bn_bwd_from_partials") else 0
    return ("vec" if vec else "scalar"), nb, ew


class Case:
    """``groups`` independent passes of B/groups images; ``capped``: both the reduction grid and the element-wise grid
    are at their caps (the exact leg only: the float leg's bound loses its teeth above 600 rows)"""

    def __init__(self, cid, B, rpi, C, route, groups=1, capped=False, why=""):
        self.id, self.B, self.rpi, self.C, self.route = cid, B, rpi, C, route
        self.groups, self.capped, self.why = groups, capped, why

    @property
    def rows(self):
        """rows of one group"""
        return self.B // self.groups * self.rpi

    @property
    def float_leg(self):
        return self.rows * self.groups <= 600 and self.rows >= 8


ROW_CASES = [
    Case("v-c8", 3, 49, 8, "vec", why="lanes_r = 128: the longest LDS fold"),
    Case("v-c12", 5, 25, 12, "vec", why="C/4 = 3 does not divide 256: lanes_r = 85, thread 255 idle"),
    Case("v-c64", 7, 25, 64, "vec", why="the shape of the older test"),
    Case("v-c256", 4, 9, 256, "vec", why="lanes_r = 4: the widest C bn_stats / bn_bwd take"),
    Case("v-cap64", 33, 2001, 64, "vec", capped=True,
         why="66033 rows: 512 reduction blocks, several trips of the 4-row loop with a ragged tail; n/4 > 524288: the "
             "apply grid strides; odd rows_per_img: image boundaries inside a quad of in-flight rows"),
    Case("v-cap256", 5, 3301, 256, "vec", capped=True, why="16505 rows: the same caps at lanes_r = 4"),
    Case("s-c6", 5, 16, 6, "scalar", why="lanes_c = 8"),
    Case("s-c1", 9, 30, 1, "scalar", why="lanes_c = 1, lanes_r = 256"),
    Case("s-c255", 2, 7, 255, "scalar", why="lanes_r = 1: the fold loop runs zero times"),
    Case("s-cap6", 3, 43700, 6, "scalar", capped=True,
         why="131100 rows > 131072: 512 reduction blocks; n > 524288: the scalar element-wise grid strides"),
    Case("g2-v64", 6, 25, 64, "vec", groups=2, why="two passes on the vec route (blockIdx.y)"),
    Case("g3-v64", 6, 25, 64, "vec", groups=3, why="three passes on the vec route"),
    Case("g2-s6", 6, 16, 6, "scalar", groups=2, why="two passes on the scalar route: one launch per group"),
    Case("n1-v4", 1, 1, 4, "vec", why="count = 1: unbiased equals biased"),
    Case("n1-s3", 1, 1, 3, "scalar", why="count = 1 on the scalar route"),
]

# bn_apply and bn_bwd_from_partials take any C (the 512-channel layers): about 40 rows each
WIDE_CASES = [
    Case("w-c768", 5, 8, 768, "vec", why="C/4 = 192: lanes_r = 1, 64 idle threads"),
    Case("w-c1024", 5, 8, 1024, "vec", why="lanes_r = 1, every thread busy: the vec cap"),
    Case("w-c1028", 5, 8, 1028, "scalar", why="above the vec cap"),
    Case("w-c510", 5, 8, 510, "scalar", why="C % 4 != 0"),
]

# ali_colsum: (id, rows, C, ld, x 16-byte aligned, route)
COLSUM_CASES = [
    ("c-ld", 147, 8, 8, True, "vec"),
    ("c-ldpad", 147, 12, 20, True, "vec"),
    ("c-ldodd", 147, 12, 13, True, "scalar"),
    ("c-300", 40, 300, 301, True, "scalar"),      # two sweeps of the scalar kernel, the second 44 channels wide
    ("c-1024", 40, 1024, 1024, True, "vec"),
    ("c-mis", 147, 64, 64, False, "scalar"),
    ("c-capv", 66033, 64, 64, True, "vec"),        # 516 blocks before the cap
    ("c-caps", 131100, 6, 7, True, "scalar"),      # 513 blocks before the cap
]

ACT_N = (1, 255, 256, 257, EW_CAP + 3)
FROM_PARTIALS_SLOTS = (1, 255, 256, 257, 700)
ALL = {c.id: c for c in ROW_CASES + WIDE_CASES}
