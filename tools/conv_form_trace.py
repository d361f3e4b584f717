#!/usr/bin/env python3
"""Launch equivalence of two builds of libdua_hip.so: issue one dua_conv3d_k3_fwd / dua_conv3d_k3_dgrad_reduce /
dua_deconv_k2s2_fwd (or _pad_fwd) per case on zero-filled buffers, under rocprofv3 --kernel-trace, once per build, and compare
the ordered lists of (kernel name with template arguments, grid, workgroup size, LDS bytes) -- they must be identical.

  rocprofv3 --kernel-trace -d <dirA> --output-format csv -- python3 tools/conv_form_trace.py run
  rocprofv3 --kernel-trace -d <dirB> --output-format csv -- python3 tools/conv_form_trace.py run lib:<path to the other build>
  python3 tools/conv_form_trace.py compare <dirA> <dirB> [summary file]

Cases (tests/conv_form_cases.py): every convolution descriptor of the pinned plans and the kernel-test regimes up to 64^3
x policy {0, 2, 3, 6, 7} x fused x workspace {none, what the form asks for, far more} x background, the 96^3 first-layer
and wide launches once each, the backward-sums launch of every descriptor that has one, and the plans' transposed convolutions
x policy {0, 6} x fused.  Workspace sizes always come from THIS tree's form query, so both builds are handed the same calls;
`lib:<path>` only replaces the library whose launchers run (as in tools/bench_conv.py).  `run` also prints one line per call
with the return code: the two logs must agree as well."""
import csv
import ctypes as C
import glob
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(argv):
    import torch
    from diff_unet_amos_amd import _native as nv
    import conv_form_cases as K
    from test_launch_sequence_fp64 import EXPECTED
    Q = nv.lib()                                     # this tree: the form queries
    L = Q
    if argv and argv[0].startswith("lib:"):
        L = C.CDLL(argv[0][4:])
        for name in ("dua_conv3d_k3_fwd", "dua_conv3d_k3_dgrad_reduce", "dua_deconv_k2s2_fwd", "dua_deconv_k2s2_pad_fwd", "dua_prepare"):
            getattr(L, name).restype, getattr(L, name).argtypes = nv._SIGS[name]
    dev = torch.device("cuda:0")
    assert L.dua_prepare() == 0
    stream = nv.stream_ptr()
    z = lambda n, dt: torch.zeros(int(n), dtype=dt, device=dev)      # noqa: E731
    calls = 0

    def producer(N, channels, count):
        cp = -(-channels // 64) * 64
        keep = (z(N * 8 * 4 * cp, torch.int64), z(cp, torch.float32), z(cp, torch.float32))
        return nv.InNorm(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), None, 0, cp, count, 1e-5, 0.1), keep

    def report(what, name, d, extra, rc):
        nonlocal calls
        calls += 1
        print(f"{what} {name} policy {d[-1]} bg {d[12]} {extra} -> {rc}", flush=True)

    def conv_cases(name, d0, policies, fuseds, backgrounds, all_ws=True):
        dt = torch.float16 if d0[0] == K.F16 else torch.float32
        N, vox, cin, cs_in, cout, cs_out = d0[1], K.voxels(d0), d0[5], d0[6], d0[8], d0[9]
        nct, nch = -(-cout // 64), -(-cin // (32 if d0[0] == K.F16 else 16))
        x, y = z(N * vox * cs_in, dt), z(N * vox * cs_out, dt)
        w = z(nct * nch * 27 * 4 * 64 * 16 + nct * 4096, torch.uint8)
        bias, stats = z(nct * 64, torch.float32), z(N * 8 * 4 * nct * 64, torch.int64)
        norm, keep = producer(N, cs_in, vox)
        needs = []
        for policy in policies:                       # what any of the policies would split into (policy 2 splits larger layers)
            f = nv.Conv3Form()
            if Q.dua_conv3d_k3_form(C.byref(nv.Conv3Desc(*K.with_fields(d0, policy=policy))), 0, 0, 0, C.byref(f)) == 0:
                needs.append(int(f.workspace_needed))
        huge = 2 * max(needs + [0]) + (1 << 20)
        ws = z(huge // 4, torch.float32)
        for policy, fused, bg in itertools.product(policies, fuseds, backgrounds):
            d = K.with_fields(d0, policy=policy, background=bg)
            desc = nv.Conv3Desc(*d)
            f = nv.Conv3Form()
            sizes = [0]
            if Q.dua_conv3d_k3_form(C.byref(desc), fused, 0, 0, C.byref(f)) == 0 and f.workspace_needed > 0 and all_ws:
                assert f.workspace_needed <= huge
                sizes += [int(f.workspace_needed), huge]
            for nbytes in sizes:
                rc = L.dua_conv3d_k3_fwd(C.byref(desc), nv.ptr(x), nv.ptr(w), nv.ptr(bias), C.byref(norm) if fused else None, nv.ptr(y),
                                         nv.ptr(stats), nv.ptr(ws) if nbytes else None, nbytes, stream)
                report("conv", name, d, f"fused {fused} ws {nbytes}", rc)
        if d0[13] == 0 and Q.dua_conv3d_k3_dgrad_reduce_supported(C.byref(nv.Conv3Desc(*d0))):
            raw, sums = z(N * vox * cs_out, dt), z(N * 8 * nct * 64 * 4, torch.float64)
            rnorm, rkeep = producer(N, cout, vox)
            for policy in policies:
                d = K.with_fields(d0, policy=policy)
                rc = L.dua_conv3d_k3_dgrad_reduce(C.byref(nv.Conv3Desc(*d)), nv.ptr(x), nv.ptr(w), nv.ptr(bias), nv.ptr(y), nv.ptr(raw),
                                                  cs_out, 0, C.byref(rnorm), nv.ptr(sums), stream)
                report("dgrad_reduce", name, d, "", rc)
        torch.cuda.synchronize()

    small = [(n, d) for n, d in K.conv_descriptors(EXPECTED) if K.voxels(d) <= 64 ** 3]
    for name, d in small:
        conv_cases(name, d, K.POLICIES, (0, 1), (0, 1))
    by_name = {n: d for n, d in K.conv_descriptors(EXPECTED)}
    conv_cases("fp16-96/d0a", by_name["fp16-96/d0a"], (0,), (0,), (0,))          # the resident-weight first layer at 96^3
    conv_cases("fp16-96/d0b", by_name["fp16-96/d0b"], (0,), (1,), (0,))          # the wide-tile form at 96^3, blocked input
    for name, d0, _, dims in K.deconv_launches(EXPECTED):
        dt = torch.float16 if d0[0] == K.F16 else torch.float32
        N, vox, cin, cs_in, cout, cs_out = d0[1], K.voxels(d0), d0[5], d0[6], d0[8], d0[9]
        nct, nch = -(-cout // 64), -(-cin // (32 if d0[0] == K.F16 else 16))
        x, y = z(N * vox * cs_in, dt), z(N * dims[0] * dims[1] * dims[2] * cs_out, dt)
        w, bias = z(8 * nct * nch * 4 * 64 * 16, torch.uint8), z(nct * 64, torch.float32)
        norm, keep = producer(N, cs_in, vox)
        padded = tuple(dims) != (2 * d0[2], 2 * d0[3], 2 * d0[4])
        for policy, fused in itertools.product((0, 6), (0, 1)):
            d = K.with_fields(d0, policy=policy)
            args = (nv.ptr(x), nv.ptr(w), nv.ptr(bias), C.byref(norm) if fused else None, nv.ptr(y), stream)
            if padded:
                rc = L.dua_deconv_k2s2_pad_fwd(C.byref(nv.Conv3Desc(*d)), *dims, *args)
            else:
                rc = L.dua_deconv_k2s2_fwd(C.byref(nv.Conv3Desc(*d)), *args)
            report("deconv_pad" if padded else "deconv", name, d, f"fused {fused}", rc)
        torch.cuda.synchronize()
    print(f"{calls} calls", flush=True)


def launches(d):
    f = (glob.glob(d + "/*/*_kernel_trace.csv") + glob.glob(d + "/*_kernel_trace.csv"))[0]
    # the library's kernels (fp16 instantiations come out mangled: _Float16 has no demangled spelling in the trace)
    rows = [r for r in csv.DictReader(open(f)) if "dua::" in r["Kernel_Name"] or r["Kernel_Name"].startswith("_ZN3dua")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    lds = [c for c in rows[0] if "LDS" in c.upper()]
    assert lds, "no LDS column in the kernel trace"
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
             r["Workgroup_Size_Z"]) + tuple(r[c] for c in lds) for r in rows]


def compare(argv):
    a, b = launches(argv[0]), launches(argv[1])
    diffs = [(i, x, y) for i, (x, y) in enumerate(itertools.zip_longest(a, b)) if x != y]
    text = (f"launches {len(a)} / {len(b)}, distinct kernels {len({r[0] for r in a})} / {len({r[0] for r in b})}, "
            f"distinct (kernel, grid, workgroup, LDS) {len(set(a))} / {len(set(b))}: {len(diffs)} differences\n")
    for i, x, y in diffs[:20]:
        text += f"  #{i}: {x}\n      {y}\n"
    by_kernel = {}
    for r in a:
        by_kernel[r[0]] = by_kernel.get(r[0], 0) + 1
    for k in sorted(by_kernel):
        text += f"  {by_kernel[k]:6d}  {k}\n"
    print(text, end="")
    if len(argv) > 2:
        open(argv[2], "w").write(text)
    return 1 if diffs or not a else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(sys.argv[2:])
    elif len(sys.argv) > 3 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2:]))
    else:
        sys.exit(__doc__)
