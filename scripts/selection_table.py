"""Every host-side answer of the convolution dispatch over a descriptor grid, as JSON: kernel id and name per op, statistics
rows, workspace / scratch / weight-gradient workspace bytes, partial-row bound, prologue support.  Two builds of the library
(PAI_HIP_LIB) that select the same kernels give equal dumps; invalid descriptors (answered -1) are part of the table.
    python scripts/selection_table.py OUT.json               no GPU needed (un-split names, no slab-dependent answers)
    python scripts/selection_table.py OUT.json --register    GPU box: workspace, scratch and weight-gradient slab registered
    python scripts/selection_table.py --diff A.json B.json   differing keys; exit status 1 when there are any
Every selection switch is a tunable; its PAI_TUNE_<name> default is read once per process: one run per setting."""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGISTER_BYTES = 1 << 30      # registration is bookkeeping: nothing launches, nothing is written

TRIPLES = [(1, 0, 64), (64, 64, 1), (16, 0, 16), (96, 0, 96), (3, 3, 64), (1, 1, 64), (32, 0, 32), (64, 0, 32), (32, 0, 64),
           (64, 0, 64), (64, 0, 128), (128, 0, 64), (64, 64, 128), (128, 0, 128), (128, 128, 64), (128, 128, 128),
           (128, 0, 256), (256, 0, 128), (64, 0, 256), (256, 0, 64), (256, 0, 1), (256, 0, 256), (256, 256, 128),
           (256, 0, 512), (512, 0, 512), (512, 512, 256), (512, 512, 512)]
KINDS = [(tr, k, s, g) for tr in (0, 1) for k, s in ((4, 2), (4, 1), (3, 1), (1, 1)) for g in ((0, 32) if k == 3 else (0,))]


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "thesis-pai-reconstruction_amd", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _desc(L, dtype, tr, k, s, g, N, H, W, C1, C2, Cout, r1, r2):
    d = L.ConvDesc()
    d.dtype, d.transposed, d.N, d.H, d.W, d.C1, d.C2, d.Cout = dtype, tr, N, H, W, C1, C2, Cout
    d.kernel, d.stride, d.pad = {4: (4, s, 1), 3: (3, 1, 1), 1: (1, 1, 0)}[k]
    d.relu1, d.relu2, d.groups = r1, r2, g
    return "dt%d tr%d k%ds%d g%d N%d %dx%d C%d+%d->%d relu%d%d" % (dtype, tr, k, s, g, N, H, W, C1, C2, Cout, r1, r2), d


def descriptors(L):
    def desc(*a):
        return _desc(L, *a)

    for dtype in (L.BF16, L.F32):
        for tr, k, s, g in KINDS:
            for N in (2, 64, 128):
                for H in (2, 4, 8, 16, 64, 256, 512):
                    for C1, C2, Cout in TRIPLES:
                        for relu in (0, 1):
                            yield desc(dtype, tr, k, s, g, N, H, H, C1, C2, Cout, relu, relu if C2 else 0)
        cases = _load_cases()
        for _, tr, s, N, H, W, C1, C2, Cout, r1, r2 in cases:
            yield desc(dtype, tr, 4, s, 0, N, H, W, C1, C2, Cout, r1, r2)


def _load_cases():
    # CASES of tests/test_gpu_conv.py without importing the module (it needs pytest and torch)
    import ast
    with open(os.path.join(ROOT, "tests", "test_gpu_conv.py")) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "CASES" for t in node.targets):
            return ast.literal_eval(node.value)
    raise RuntimeError("tests/test_gpu_conv.py: CASES not found")


def dump(path, register):
    if register:
        import torch      # before the library, as in the package: one HIP runtime for both
    L = _load("lib")
    lib = L.load()
    keep = []
    if register:
        for fn in (lib.pai_set_workspace, lib.pai_set_scratch, lib.pai_set_wgrad_workspace):
            keep.append(torch.zeros(REGISTER_BYTES, dtype=torch.uint8, device="cuda:0"))
            L.check(fn(keep[-1].data_ptr(), REGISTER_BYTES), "register")
    buf = C.create_string_buffer(96)
    table = {}
    for key, d in descriptors(L):
        p = C.byref(d)
        row = {}
        for op in (0, 1, 2):
            row["id%d" % op] = lib.pai_conv_kernel_id(p, op)
            row["name%d" % op] = buf.value.decode() if lib.pai_conv_kernel_name(p, op, buf, 96) == 0 else None
            row["workspace%d" % op] = lib.pai_conv_workspace_bytes(p, op)
            row["scratch%d" % op] = lib.pai_conv_scratch_bytes(p, op)
        row["stats_rows"] = lib.pai_conv_fwd_stats_rows(p)
        row["stats_rows_max"] = lib.pai_conv_fwd_stats_rows_max(p)
        row["wgrad_workspace"] = lib.pai_conv_wgrad_workspace_bytes(p)
        row["dgrad_bn_rows_max"] = lib.pai_conv_dgrad_bn_rows_max(p)
        row["prologue_ok"] = lib.pai_conv_prologue_ok(p)
        table[key] = row
    # pai_conv_dgrad_act_wthin takes a PAIR of layers (thin first layer, the layer behind): rows of their own, for a library
    # that has the entry point
    if hasattr(lib, "pai_conv_dgrad_act_wthin_ok"):
        for dtype in (L.BF16, L.F32):
            for N in (2, 64, 128):
                for H, W in ((32, 64), (64, 64), (256, 256), (96, 160)):
                    for T in (1, 2):
                        d0 = _desc(L, dtype, 0, 4, 2, 0, N, H, W, 1, T - 1, 64, 0, 0)[1]
                        d1 = _desc(L, dtype, 0, 4, 2, 0, N, H // 2, W // 2, 64, 0, 128, 0, 0)[1]
                        ok = lib.pai_conv_dgrad_act_wthin_ok(C.byref(d1), C.byref(d0), 0)
                        named = lib.pai_conv_dgrad_act_wthin_kernel_name(C.byref(d1), C.byref(d0), buf, 96) == 0
                        table["wthin:%d:%d:%d:%d:%d" % (dtype, N, H, W, T)] = {
                            "ok": ok, "name": buf.value.decode() if named else None,
                            "slab_bytes": lib.pai_conv_dgrad_act_wthin_slab_bytes(C.byref(d1), C.byref(d0))}
    text = json.dumps(table, sort_keys=True, indent=0)
    with open(path, "w") as f:
        f.write(text)
    layers = [r for r in table.values() if "id0" in r]
    names = ({r["name%d" % op] for r in layers for op in (0, 1, 2)} | {r.get("name") for r in table.values()}) - {None}
    ids = {r["id%d" % op] for r in layers for op in (0, 1)}
    print(json.dumps({"lib": L.LIB_PATH, "rows": len(table), "invalid": sum(r["id0"] < 0 for r in layers),
                      "names": len(names), "ids_op01": sorted(ids), "sha256": hashlib.sha256(text.encode()).hexdigest()}))


def diff(a, b):
    with open(a) as f:
        A = json.load(f)
    with open(b) as f:
        B = json.load(f)
    bad = 0
    for key in sorted(set(A) | set(B)):
        ra, rb = A.get(key), B.get(key)
        if ra == rb:
            continue
        bad += 1
        if ra is None or rb is None:
            print("%s: only in %s" % (key, a if rb is None else b))
        else:
            print("%s: %s" % (key, ", ".join("%s %r != %r" % (k, ra.get(k), rb.get(k)) for k in sorted(set(ra) | set(rb))
                                             if ra.get(k) != rb.get(k))))
    print("%d of %d rows differ" % (bad, len(set(A) | set(B))))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    if len(sys.argv) < 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    dump(sys.argv[1], "--register" in sys.argv[2:])
