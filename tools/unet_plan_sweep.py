#!/usr/bin/env python3
"""The plan of every supported network as text, digested - host code only, no device needed.  The companion of conv_plan_sweep.py.

    python tools/unet_plan_sweep.py LIB [--dump DIR]

LIB is a libvolseg_hip.so.  For each of the 56 (topology 0-7, encoder 18 / 34 / 50 / 51 / 103 / 104 / 150 / 201) pairs that
vs_unet_create_ex accepts, the plan is created for dtype fp32 / bf16 / fp16 x classes 1 / 3 / 16 x (max_batch, h, w) (1, 32, 32) /
(2, 64, 96) / (32, 256, 256) and written out by vs_unet_plan_dump: every field of the plan, its tensors, activations and units.  One
SHA-256 per pair over its 27 dumps, in that order, and one over everything.  The sweep runs under the default options and refuses to
run under any other.  --dump DIR writes the texts as DIR/<code>/<dtype>_<classes>_<batch>x<h>x<w>.txt.

Two builds construct the same plans, field for field and byte offset for byte offset, exactly when every digest line matches; where
one does not, `diff -r` of the two --dump trees names the field.
"""
import ctypes as C
import hashlib
import itertools
import sys
from pathlib import Path

TOPOLOGIES = range(8)
ENCODERS = (18, 34, 50, 51, 103, 104, 150, 201)
DTYPES = ((0, "fp32"), (1, "bf16"), (2, "fp16"))
CLASSES = (1, 3, 16)
SIZES = ((1, 32, 32), (2, 64, 96), (32, 256, 256))
DEFAULT_OPTIONS = dict(   # csrc/prof.hip: g_opts
    side_stream=1, conv_direct=1, conv_nw8=1, conv_ring=1, conv_stream=1, wgrad_ring=1, wgrad_xcd=1, stats_bins=1, fuse_bn_bwd=1, nl_fwd=1,
    stem_bf16=1, conv_pair=1, conv_min_wgs=512, conv_nw8_min_wgs=128, conv_direct_min_px=262144, conv_direct_rows=32,
    conv_direct_rows_big=128, conv_ring_max_wgs=1024, conv_stream_min_tiles=2, wgrad_target=96, wgrad_target_plain=256, wgrad_slab_mb=16,
    fork_every=2, bn_inline_rows=64, nl_max_c=64, bn_prefetch=1)


_BUF = C.create_string_buffer(1 << 20)   # one dump fits (the largest of the sweep is under 0.4 MB); a larger one is asked for again


def load(path):
    lib = C.CDLL(str(path))
    for name, res, args in (("vs_unet_create_ex", C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 6), ("vs_unet_destroy", None, [C.c_void_p]),
                            ("vs_unet_plan_dump", C.c_size_t, [C.c_void_p, C.c_char_p, C.c_size_t]), ("vs_get_option", C.c_int, [C.c_char_p])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def plan_text(lib, dtype, classes, batch, h, w, code):
    """the dump of one plan, or None where vs_unet_create_ex refuses the code"""
    net = C.c_void_p()
    if lib.vs_unet_create_ex(C.byref(net), dtype, classes, batch, h, w, code):
        return None
    try:
        need = lib.vs_unet_plan_dump(net, _BUF, len(_BUF))
        if need <= len(_BUF):
            return _BUF.raw[:need]
        buf = C.create_string_buffer(need)
        assert lib.vs_unet_plan_dump(net, buf, need) == need
        return buf.raw
    finally:
        lib.vs_unet_destroy(net)


def sweep(lib, dump_dir=None):
    """{code: sha256 hex digest over the 27 plans of the pair}, for every accepted pair, in code order"""
    changed = {k: lib.vs_get_option(k.encode()) for k, v in DEFAULT_OPTIONS.items() if lib.vs_get_option(k.encode()) != v}
    assert not changed, f"the plan sweep runs under the default options only: {changed}"
    digests = {}
    for code in (t * 1000 + e for t in TOPOLOGIES for e in ENCODERS):
        if plan_text(lib, 0, 1, *SIZES[0], code) is None:     # (not a supported pair)
            continue
        sha = hashlib.sha256()
        for (dtype, dname), classes, (batch, h, w) in itertools.product(DTYPES, CLASSES, SIZES):
            text = plan_text(lib, dtype, classes, batch, h, w, code)
            assert text is not None, (code, dname, classes, batch, h, w)
            sha.update(text)
            if dump_dir is not None:
                out = Path(dump_dir) / f"{code:04d}" / f"{dname}_{classes}_{batch}x{h}x{w}.txt"
                out.parent.mkdir(parents=True, exist_ok=True)
                out.write_bytes(text)
        digests[code] = sha.hexdigest()
    return digests


def main():
    args = sys.argv[1:]
    dump_dir = None
    if "--dump" in args:
        i = args.index("--dump")
        dump_dir = args[i + 1]
        del args[i:i + 2]
    if len(args) != 1:
        sys.exit(__doc__)
    digests = sweep(load(args[0]), dump_dir)
    total = hashlib.sha256()
    for code, digest in digests.items():
        print(f"{code:04d} {digest}")
        total.update(f"{code} {digest}\n".encode())
    print(f"== {len(digests)} pairs x {len(DTYPES) * len(CLASSES) * len(SIZES)} plans, sha256 {total.hexdigest()}")


if __name__ == "__main__":
    main()
