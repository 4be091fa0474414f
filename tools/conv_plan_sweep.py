#!/usr/bin/env python3
"""Which kernel every convolution launch gets, swept over a product of descriptors - host code only, no device needed.

    python tools/conv_plan_sweep.py LIB [--quick]

LIB is a libvolseg_hip.so.  For every descriptor the pure host queries of the C ABI are asked - vs_conv2d_variant,
vs_conv2d_wgrad_workspace and, with four training blocks (none, stats_partial, stats_bins, pool0), vs_conv2d_train_variant and
vs_conv2d_stat_rows - and every returned value goes into a SHA-256.  A second, smaller product adds split outputs, grouped layers,
the BN-backward epilogue, normalise-on-load and pairs of layers (vs_conv2d_pair_ok).  Both products run with the default options and again
under each of conv_direct=0, conv_ring=0, conv_stream=0, conv_nw8=0, conv_pair=0 and conv_min_wgs=64.  --quick: two batch sizes
instead of five in the first product.

Two builds choose the same kernels everywhere exactly when every digest line matches: run it on both and compare the output.
"""
import ctypes as C
import hashlib
import itertools
import struct
import sys
from collections import Counter


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "dtype", "n", "hin", "win", "c0", "c1", "up0", "cout", "kh", "kw", "stride", "pad", "relu", "out_f32", "split_c", "groups", "dilation")]


class ConvTrain(C.Structure):
    _fields_ = [("stats_bins", C.c_void_p), ("stats_nb", C.c_int32), ("stats_partial", C.c_void_p), ("pool0", C.c_int32),
                ("bz", C.c_void_p), ("by", C.c_void_p), ("bmean", C.c_void_p), ("binvstd", C.c_void_p), ("bgamma", C.c_void_p),
                ("bbeta", C.c_void_p), ("bstats_partial", C.c_void_p), ("brelu", C.c_int32),
                ("nl_bins", C.c_void_p), ("nl_nb", C.c_int32), ("nl_rows", C.c_int64), ("nl_eps", C.c_float), ("nl_mom", C.c_float),
                ("nl_mean", C.c_void_p), ("nl_invstd", C.c_void_p), ("nl_rm", C.c_void_p), ("nl_rv", C.c_void_p),
                ("nl_gamma", C.c_void_p), ("nl_beta", C.c_void_p), ("nl_y", C.c_void_p)]


FAKE = 16   # the queries never dereference a pointer
KSD = ((1, 1, 1), (1, 2, 1), (3, 1, 1), (3, 2, 1), (3, 1, 2))   # (kernel, stride, dilation): dilation 2 is a stride-1 3x3 form


def load(path):
    lib = C.CDLL(path)
    dp, tp = C.POINTER(ConvDesc), C.POINTER(ConvTrain)
    for name, res, args in (("vs_conv2d_variant", C.c_int, [dp]), ("vs_conv2d_train_variant", C.c_int, [dp, tp]),
                            ("vs_conv2d_stat_rows", C.c_int, [dp, tp]), ("vs_conv2d_pair_ok", C.c_int, [dp, dp]),
                            ("vs_conv2d_wgrad_workspace", C.c_size_t, [dp]), ("vs_set_option", C.c_int, [C.c_char_p, C.c_int]),
                            ("vs_get_option", C.c_int, [C.c_char_p])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def train_blocks(extended):
    blocks = [("none", ConvTrain()), ("stats_partial", ConvTrain(stats_partial=FAKE)), ("stats_bins", ConvTrain(stats_bins=FAKE, stats_nb=8)),
              ("pool0", ConvTrain(pool0=1))]
    if extended:
        bz = dict(bz=FAKE, bmean=FAKE, binvstd=FAKE, bgamma=FAKE, bbeta=FAKE, bstats_partial=FAKE, brelu=1)
        nl = dict(nl_bins=FAKE, nl_nb=8, nl_rows=4096, nl_eps=1e-5, nl_mom=0.1, nl_mean=FAKE, nl_invstd=FAKE, nl_rm=FAKE, nl_rv=FAKE,
                  nl_gamma=FAKE, nl_beta=FAKE, nl_y=FAKE)
        blocks += [("bz", ConvTrain(**bz)), ("bz+by", ConvTrain(by=FAKE, **bz)), ("nl", ConvTrain(**nl)),
                   ("nl+stats_bins", ConvTrain(stats_bins=FAKE, stats_nb=8, **nl)), ("nl+stats_partial", ConvTrain(stats_partial=FAKE, **nl))]
    return blocks


class Sweep:
    def __init__(self, lib):
        self.lib, self.sha, self.cases, self.codes = lib, hashlib.sha256(), 0, Counter()

    def desc(self, d, blocks):
        lib = self.lib
        vals = [lib.vs_conv2d_variant(d), lib.vs_conv2d_wgrad_workspace(d)]
        self.codes[vals[0]] += 1
        for _, t in blocks:
            vals += [lib.vs_conv2d_train_variant(d, t), lib.vs_conv2d_stat_rows(d, t)]
        self.sha.update(struct.pack(f"<{len(vals)}q", *vals))
        self.cases += 1

    def pair(self, d1, d2):
        self.sha.update(struct.pack("<q", self.lib.vs_conv2d_pair_ok(d1, d2)))
        self.cases += 1

    def report(self, title):
        kinds = Counter()
        for code, k in self.codes.items():
            kinds[code % 10 if code >= 0 else code] += k
        print(f"== {title}: {self.cases} cases, sha256 {self.sha.hexdigest()}")
        print("   last digit / error: " + ", ".join(f"{d}: {k}" for d, k in sorted(kinds.items())))
        print("   codes: " + ", ".join(f"{c}: {k}" for c, k in sorted(self.codes.items())))


def pow2(lo, hi):
    return [1 << i for i in range(lo.bit_length() - 1, hi.bit_length())]


def base_product(lib, quick):
    s = Sweep(lib)
    blocks = train_blocks(False)
    ns = (2, 32) if quick else (1, 2, 12, 32, 128)
    for dtype, n, hw, c0, c1, up0, cout, (k, stride, dil), out_f32 in itertools.product(
            (0, 1, 2), ns, pow2(8, 512), pow2(8, 512), (0, 32, 64), (0, 1), (4, 16, 32, 64, 128, 256, 512), KSD, (0, 1, 3)):
        s.desc(ConvDesc(dtype=dtype, n=n, hin=hw, win=hw, c0=c0, c1=c1, up0=up0, cout=cout, kh=k, kw=k, stride=stride,
                        pad=dil * (k // 2), out_f32=out_f32, dilation=dil), blocks)
    return s


def extended_product(lib):
    """split outputs, grouped layers, the BN-backward epilogue, normalise-on-load (all with every training block), then pairs"""
    s = Sweep(lib)
    blocks = train_blocks(True)
    for dtype, n, hw, c0, c1, cout, (k, stride, dil), up0 in itertools.product(
            (0, 1, 2), (2, 12, 32), (8, 16, 64, 256), (16, 32, 64, 128, 256), (0, 64), (16, 32, 64, 96, 128, 256), KSD, (0, 1, 2)):
        common = dict(dtype=dtype, n=n, hin=hw, win=hw, c0=c0, c1=c1, up0=up0, cout=cout, kh=k, kw=k, stride=stride, pad=dil * (k // 2), dilation=dil)
        s.desc(ConvDesc(**common), blocks)
        for split_c in (16, 32, 48, 64):
            if split_c < cout:
                s.desc(ConvDesc(split_c=split_c, **common), blocks)
        if c0 == cout and not c1:
            for groups in (c0 // 4, c0 // 8, c0 // 32):
                if groups > 1:
                    s.desc(ConvDesc(groups=groups, **common), blocks)
        if dil == 1 and stride == 1 and k == 3:
            s.desc(ConvDesc(**{**common, "pad": 4, "dilation": 4}), blocks)
    for dtype, n, hw, c0, cmid, cout, relu, f32 in itertools.product(
            (0, 1, 2), (1, 12, 128), (32, 64, 256, 512), (8, 16, 32), (8, 12, 16, 32), (4, 8, 16, 32), (0, 1), (0, 1)):
        d1 = ConvDesc(dtype=dtype, n=n, hin=hw, win=hw, c0=c0, cout=cmid, kh=3, kw=3, stride=1, pad=1, relu=relu, dilation=1)
        d2 = ConvDesc(dtype=dtype, n=n, hin=hw, win=hw, c0=cmid, cout=cout, kh=3, kw=3, stride=1, pad=1, relu=relu, out_f32=f32, dilation=1)
        s.pair(d1, d2)
    return s


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1:
        sys.exit(__doc__)
    quick = "--quick" in sys.argv
    lib = load(args[0])
    base_product(lib, quick).report("base product, default options")
    extended_product(lib).report("extended product, default options")
    for name, value in (("conv_direct", 0), ("conv_ring", 0), ("conv_stream", 0), ("conv_nw8", 0), ("conv_pair", 0), ("conv_min_wgs", 64)):
        default = lib.vs_get_option(name.encode())
        if lib.vs_set_option(name.encode(), value):
            sys.exit(f"vs_set_option({name}) failed")
        base_product(lib, quick).report(f"base product, {name}={value}")
        extended_product(lib).report(f"extended product, {name}={value}")
        lib.vs_set_option(name.encode(), default)


if __name__ == "__main__":
    main()
