"""CPU checks of the fused Adam step (adam.hip, hs_adam_*, casualhdrsplat_amd.optim): the C ABI (exports, struct layout,
argument validation before any HIP call), the Python argument errors and state_dict layout, the numpy restatement the GPU
tests compare bits with (tests/adam_reference.py) pinned against torch.optim.Adam, and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import adam_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hs_adam_state_bytes", "hs_adam_step")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "casualhdrsplat_amd", "csrc"), "-j4"])
    from casualhdrsplat_amd import _lib
    return _lib


# ---- C ABI ----

def test_adam_symbols_are_declared_and_exported_by_both_libraries(lib):
    header = open(os.path.join(ROOT, "include", "hdrsplat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert re.search(rf"\bHS_API\s+\w+\s+{n}\s*\(", header), n
    assert set(NAMES) <= set(lib.EXPORTS)
    for path in (lib.LIB_PATH, os.path.join(os.path.dirname(lib.LIB_PATH), "libhdrsplat_test.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for n in NAMES:
            assert re.search(rf"\bT {n}\b", out), (path, n)
    assert lib.load().hs_version() == 309        # (detected by name: the version does not move)


def test_adam_structs_match_c(lib, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdrsplat.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(hs_adam_group), sizeof(hs_adam_args),'
                   'offsetof(hs_adam_group, rows), offsetof(hs_adam_group, masked), offsetof(hs_adam_args, mask_kind),'
                   'offsetof(hs_adam_args, mask), offsetof(hs_adam_args, state), offsetof(hs_adam_args, hyper),'
                   'HS_ADAM_MAX_GROUPS, HS_ADAM_MASK_NONE, HS_ADAM_MASK_RADII, HS_ADAM_MASK_BYTES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    G, A = lib.hs_adam_group, lib.hs_adam_args
    assert got == [C.sizeof(G), C.sizeof(A), G.rows.offset, G.masked.offset, A.mask_kind.offset, A.mask.offset, A.state.offset,
                   A.hyper.offset, lib.HS_ADAM_MAX_GROUPS, lib.HS_ADAM_MASK_NONE, lib.HS_ADAM_MASK_RADII, lib.HS_ADAM_MASK_BYTES]


def test_state_bytes(lib):
    L = lib.load()
    for n in (1, 5, 16):
        assert L.hs_adam_state_bytes(n) == 64 + 64 * n
    for n in (0, -1, 17):
        assert L.hs_adam_state_bytes(n) == lib.HS_EINVAL
        assert b"hs_adam_state_bytes" in L.hs_last_error() and f"n_groups={n}".encode() in L.hs_last_error()


def test_adam_step_validates_before_touching_the_gpu(lib):
    """Every argument error is HS_EINVAL with a message that names the field -- on a machine without a GPU: no HIP call is
    made before the arguments are known to be good."""
    L = lib.load()
    one = 4096     # non-null dummy addresses: validation must fail before any of them is dereferenced

    def call(n=2, group=None, **kw):
        groups = (lib.hs_adam_group * max(n, 1))()
        for i in range(max(n, 1)):
            g = groups[i]
            g.param = g.grad = g.exp_avg = g.exp_avg_sq = one
            g.rows, g.row_stride, g.col_begin, g.col_count, g.masked = 100, 48, 0, 48, 1
        for k, v in (group or {}).items():
            setattr(groups[n - 1], k, v)
        a = lib.hs_adam_args()
        a.groups, a.n_groups = groups, n
        a.mask_kind, a.mask, a.mask_len = lib.HS_ADAM_MASK_RADII, one, 100
        a.state, a.hyper = one, one
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.hs_adam_step(C.byref(a), None)
        return rc, L.hs_last_error()

    assert L.hs_adam_step(None, None) == lib.HS_EINVAL and b"null args" in L.hs_last_error()
    cases = [
        (dict(n=0), b"n_groups=0"), (dict(n=17), b"n_groups=17"), (dict(n_groups=-3), b"n_groups=-3"),
        (dict(groups=None), b"null groups"), (dict(state=None), b"null state"), (dict(hyper=None), b"null hyper"),
        (dict(state=one + 8), b"state must be 16-byte aligned"), (dict(hyper=one + 4), b"hyper must be 8-byte aligned"),
        (dict(mask_kind=3), b"mask_kind=3"), (dict(mask_kind=-1), b"mask_kind=-1"),
        (dict(mask_len=-5), b"mask_len=-5"), (dict(mask=None), b"null mask"),
        (dict(mask_len=99), b"groups[0].rows=100 differs from mask_len=99"),
        (dict(group=dict(rows=-1)), b"groups[1].rows=-1"),
        (dict(group=dict(row_stride=0)), b"groups[1]: row_stride=0"),
        (dict(group=dict(col_begin=-1)), b"col_begin=-1"),
        (dict(group=dict(col_count=0)), b"col_count=0"),
        (dict(group=dict(col_begin=40, col_count=9)), b"groups[1]: col_begin + col_count > row_stride (40 + 9 > 48)"),
        (dict(group=dict(col_begin=49, col_count=1)), b"col_begin + col_count > row_stride"),
        (dict(group=dict(rows=1 << 36, row_stride=1 << 5, col_count=1 << 5), mask_kind=0), b"exceeds 2^40"),
        (dict(group=dict(rows=101)), b"groups[1].rows=101 differs from mask_len=100"),
        (dict(group=dict(param=None)), b"groups[1]: null param"),
        (dict(group=dict(grad=None)), b"groups[1]: null param/grad"),
        (dict(group=dict(exp_avg=None)), b"null param/grad/exp_avg"),
        (dict(group=dict(exp_avg_sq=None)), b"exp_avg_sq"),
        (dict(group=dict(grad=one + 2)), b"4-byte aligned"),
    ]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == lib.HS_EINVAL, (kw, rc, msg)
        assert msg.startswith(b"hs_adam_step") and text in msg, (kw, msg)


# ---- Python ----

def test_python_argument_errors():
    from casualhdrsplat_amd import GaussianAdam, cloud_param_groups, optim
    assert optim.GaussianAdam is GaussianAdam and optim.cloud_param_groups is cloud_param_groups
    x = torch.zeros(8, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GaussianAdam([x])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GaussianAdam(cloud_param_groups(x, x.clone(), torch.zeros(8, 4, 3), x.clone(), torch.zeros(8, 4)))
    with pytest.raises(ValueError, match="weight_decay"):
        GaussianAdam([x], weight_decay=0.1)
    with pytest.raises(ValueError, match="weight_decay"):
        GaussianAdam([dict(params=[x], weight_decay=1e-3)])
    with pytest.raises(ValueError, match="amsgrad"):
        GaussianAdam([x], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        GaussianAdam([x], maximize=True)
    with pytest.raises(TypeError, match="float32"):
        GaussianAdam([torch.zeros(8, 3, dtype=torch.float16)])
    with pytest.raises(TypeError, match="float32"):
        GaussianAdam([torch.zeros(8, 3, dtype=torch.float64)])
    # visibility: dtype, shape and LENGTH are looked at before the device
    with pytest.raises(ValueError, match="length 7.*8 rows"):
        optim.check_visibility(torch.zeros(7, dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="length 9.*8 rows"):
        optim.check_visibility(torch.zeros(9, dtype=torch.bool), 8)
    with pytest.raises(TypeError, match="int32 radii or a bool"):
        optim.check_visibility(torch.zeros(8), 8)
    with pytest.raises(ValueError, match="one entry per Gaussian"):
        optim.check_visibility(torch.zeros(8, 1, dtype=torch.bool), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.check_visibility(torch.zeros(8, dtype=torch.bool), 8)


def _host_optimizer(monkeypatch, groups, **kw):
    """A GaussianAdam over CPU tensors with the device guard lifted: its host-side bookkeeping (groups, tables, state
    dicts) is plain torch and can be looked at without a GPU.  Nothing here launches a kernel."""
    from casualhdrsplat_amd import optim
    monkeypatch.setattr(optim, "_require_gpu", lambda t, what: None)
    return optim.GaussianAdam(groups, **kw)


def test_one_tensor_in_two_column_groups_and_overlaps(monkeypatch):
    from casualhdrsplat_amd import cloud_param_groups
    P = 10
    t = {k: torch.zeros(P, *s, requires_grad=True) for k, s in (("means3D", (3,)), ("opacities", (1,)), ("shs", (16, 3)),
                                                                  ("scales", (3,)), ("rotations", (4,)))}
    opt = _host_optimizer(monkeypatch, cloud_param_groups(**t), eps=1e-15)
    assert [g["name"] for g in opt.param_groups] == ["xyz", "opacity", "f_dc", "f_rest", "scaling", "rotation"]
    dc, rest = opt.param_groups[2], opt.param_groups[3]
    assert dc["params"][0] is rest["params"][0] and dc["columns"] == (0, 3) and rest["columns"] == (3, 48)
    assert abs(dc["lr"] / rest["lr"] - 20.0) < 1e-9 and all(g["per_gaussian"] and g["eps"] == 1e-15 for g in opt.param_groups)
    assert opt._matrix(t["shs"], rest) == (P, 48, 3, 45) and opt._matrix(t["opacities"], opt.param_groups[1]) == (P, 1, 0, 1)
    with pytest.raises(ValueError, match="overlapping columns"):
        opt.add_param_group(dict(params=[t["shs"]], columns=(2, 5)))
    with pytest.raises(ValueError, match="more than one parameter group"):
        opt.add_param_group(dict(params=[t["means3D"]]))
    with pytest.raises(ValueError, match="outside the 48 columns"):
        _host_optimizer(monkeypatch, [dict(params=[t["shs"]], columns=(40, 49))])
    # a dense group of anything: rows = numel, one column
    extra = torch.zeros(5, 7, requires_grad=True)
    opt.add_param_group(dict(params=[extra], lr=1e-3))
    assert opt._matrix(extra, opt.param_groups[-1]) == (35, 1, 0, 1)


def test_state_dict_keys_and_shapes_are_torchs(monkeypatch, lib):
    a, b = torch.randn(6, 3), torch.randn(4)
    pa, pb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = torch.optim.Adam([dict(params=[pa], lr=1e-2), dict(params=[pb], lr=3e-3)], eps=1e-15)
    for _ in range(3):
        pa.grad, pb.grad = torch.randn_like(pa), torch.randn_like(pb)
        ref.step()
    want = ref.state_dict()
    qa, qb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    opt = _host_optimizer(monkeypatch, [dict(params=[qa], lr=1e-2, per_gaussian=True), dict(params=[qb], lr=3e-3)], eps=1e-15)
    opt.prepare()
    got = opt.state_dict()
    assert sorted(got) == sorted(want) == ["param_groups", "state"]
    assert sorted(got["state"]) == sorted(want["state"]) == [0, 1]
    for i in (0, 1):
        assert sorted(got["state"][i]) == sorted(want["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert got["state"][i][k].shape == want["state"][i][k].shape and got["state"][i][k].dtype == want["state"][i][k].dtype
    assert [g["params"] for g in got["param_groups"]] == [g["params"] for g in want["param_groups"]] == [[0], [1]]
    for g, w in zip(got["param_groups"], want["param_groups"]):
        assert {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"} <= set(g) and g["lr"] == w["lr"] and g["eps"] == w["eps"]
    # torch's dict loads: moments adopted, the step count and the products beta^t (pow) seeded into the device table
    opt.load_state_dict(want)
    assert opt._read_t() == 3
    assert torch.equal(opt.state[qa]["exp_avg"], ref.state[pa]["exp_avg"]) and torch.equal(opt.state[qb]["exp_avg_sq"], ref.state[pb]["exp_avg_sq"])
    assert opt.param_groups[0]["per_gaussian"] is True and opt.param_groups[1]["per_gaussian"] is False
    blob = opt._dev_state.numpy().tobytes()
    assert len(blob) == lib.load().hs_adam_state_bytes(2)
    assert np.frombuffer(blob, dtype=np.float64, count=2, offset=64).tolist() == [0.9 ** 3, 0.999 ** 3]
    assert float(opt.state_dict()["state"][0]["step"]) == 3.0
    # ... and ours loads into torch
    ref.load_state_dict(opt.state_dict())
    # parameters at different steps cannot be expressed
    want["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="one step count"):
        opt.load_state_dict(want)


# ---- the restatement ----

def test_the_reference_is_as_close_to_fp64_adam_as_fp32_torch_is():
    """50 steps on [20000, 48], gradients spanning 1e-8 .. 1 in scale with 5 % exact zeros, eps = 1e-15: the restatement's
    error against torch.optim.Adam in float64 (max and RMS over elements) is at most 1.5 x the error of torch.optim.Adam in
    float32 on the same inputs.  Two valid fp32 rounding orders do not differ by 1.5 x; a wrong formula does."""
    p0, grads = R.pinned_case()
    lr, b1, b2, eps = R.PINNED_HYPER

    def run_torch(dtype):
        p = torch.tensor(p0, dtype=dtype).requires_grad_(True)
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
        for g in grads:
            p.grad = torch.tensor(g, dtype=dtype)
            opt.step()
        return p.detach().double().numpy()

    truth, t32 = run_torch(torch.float64), run_torch(torch.float32)
    p = p0.copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    st = R.AdamReference(1)
    for g in grads:
        (d,) = st.tick([R.PINNED_HYPER])
        R.update(p, g, m, v, d)
    assert st.t == 50
    e_ref, e_t32 = p.astype(np.float64) - truth, t32 - truth
    move = float(np.sqrt(np.mean((truth - p0) ** 2)))
    mx = (float(np.abs(e_ref).max()), float(np.abs(e_t32).max()))
    rms = (float(np.sqrt(np.mean(e_ref ** 2))), float(np.sqrt(np.mean(e_t32 ** 2))))
    print(f"max error: reference {mx[0]:.3e}, torch fp32 {mx[1]:.3e} (ratio {mx[0] / mx[1]:.4f}); RMS {rms[0]:.3e} / {rms[1]:.3e} "
          f"(ratio {rms[0] / rms[1]:.4f}); RMS movement {move:.3e}")
    assert move > 1e-3
    assert mx[0] <= 1.5 * mx[1] and rms[0] <= 1.5 * rms[1], (mx, rms)


def test_reference_sparse_rule_and_running_products():
    rng = np.random.default_rng(1)
    p = rng.standard_normal((9, 5)).astype(np.float32)
    g = rng.standard_normal((9, 5)).astype(np.float32)
    m, v = (0.1 * g).astype(np.float32), (0.5 * g * g).astype(np.float32)
    p0, m0, v0 = p.copy(), m.copy(), v.copy()
    vis = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], dtype=bool)
    st = R.AdamReference(2)
    hyper = [(1e-2, 0.9, 0.999, 1e-8), (1e-3, 0.8, 0.99, 1e-15)]
    d = st.tick(hyper)
    d = st.tick(hyper)
    assert st.t == 2 and st.B1 == [0.9 * 0.9, 0.8 * 0.8] and st.B2 == [0.999 * 0.999, 0.99 * 0.99]
    assert d[1].step_size == np.float32(1e-3 / (1.0 - 0.8 * 0.8)) and d[0].omb2 == np.float32(1.0 - 0.999) == np.float32(0.001)
    R.update(p, g, m, v, d[0], vis)
    for x, x0 in ((p, p0), (m, m0), (v, v0)):
        assert R.same_bits(x[~vis], x0[~vis]) and not np.any(x[vis] == x0[vis])
    # dense Adam with a zero gradient is something else: the moments decay and the momentum moves the row
    q, mq, vq = p0.copy(), m0.copy(), v0.copy()
    R.update(q, np.zeros_like(g), mq, vq, d[0])
    assert not np.any(q == p0) and not np.any(mq == m0)
    assert R.same_bits(np.array([np.nan, 1.0], np.float32), np.array([np.nan, 1.0], np.float32))
    assert not R.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))


# ---- resources ----

def test_adam_kernels_spill_nothing_need_no_scratch_and_keep_denormals():
    src = os.path.join(ROOT, "casualhdrsplat_amd", "csrc", "adam.hip")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "adam.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-fvisibility=hidden", "-std=c++17",
                            "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", src,
                            "-o", asm], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(asm).read()
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert sorted(k.split("_kernel")[0][-9:] for k in out) == ["adam_tick", "am_update"], sorted(out)
    for k, v in out.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
    upd = next(v for k, v in out.items() if "adam_update_kernel" in k)
    assert upd["Occupancy"] >= 8 and upd["VGPRs"] <= 64, upd
    # the code object: no private segment, fp32 denormals kept (mode 3 = no flush, sources and results), 16-byte accesses,
    # IEEE division (the scale / fmas / fixup sequence) -- and neither atomics nor LDS
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0", "0"]
    assert re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", text) == ["3", "3"]
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text and re.search(r"global_store_dwordx4 .* nt\b", text)
    assert "v_div_fixup_f32" in text and "v_div_scale_f32" in text and "v_sqrt_f32" in text
    assert "atomic" not in text and "ds_write" not in text and "scratch_" not in text
