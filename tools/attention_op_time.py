"""Times the Attention operator's kernel paths (hip/attention.hip: is_causal, grouped heads) and RmsNorm beside what was there before,
device-resident, 16,384 rows, T = 128, 8 heads x 16.  Every attention model reads ONE packed input [N, T (hq + 2 hkv) dh] whose Split is
absorbed, so every plan is the Attention step alone:
  (1) the unmasked pattern-form model on a build of the parent commit (--parent-lib) and on this one, alternating, three times each: the
      same kernel text for that instantiation, so the difference must lie inside the spread of the parent's own repeated runs;
  (2) the pattern form with the constant [T, T] causal mask (parent and this) beside the operator with is_causal (this): what skipping saves;
  (3) the operator with hkv = 8, 2 and 1 (hq = 8);
  (4) RmsNorm beside LayerNorm at E = 64 and E = 768, in TB/s of its 8 bytes per element;
  (5) torch-ROCm float32 scaled_dot_product_attention(is_causal=True) on the same tensors, for orientation.
A library is chosen when a process starts (INFERA_LIB_PATH), so each leg is a child process of this one, one at a time; REPS timed
repetitions of 3 calls after a warm call, medians.
usage (GPU box): python tools/attention_op_time.py [--parent-lib ab/parent/libinfera.so]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())

REPS, ROWS, T, HQ, DH = 7, 16384, 128, 8, 16
E = HQ * DH


def pattern_graph(W, causal):
    return W.attention_only(T, E, HQ, form="packed", mask=W.causal_mask(T) if causal else None)


def op_graph(W, hkv, causal):
    ekv = hkv * DH
    nodes = [W.node("Reshape", ["X", "x_shape"], ["X3"]), W.node("Split", ["X3", "sp"], ["q", "k", "v"], [W.attr_i("axis", 2)], name="split_qkv")]
    inits = [W.tensor("x_shape", np.asarray([-1, T, E + 2 * ekv], dtype=np.int64)), W.tensor("sp", np.asarray([E, ekv, ekv], dtype=np.int64))]
    out = W.attention_op_nodes(nodes, inits, "a_", "q", "k", "v", T, T, HQ, hkv, DH, causal=causal)
    return W.model("attention_op", nodes, inits, [W.value_info("X", ["N", T * (E + 2 * ekv)])], [W.value_info(out, ["N", T, E])], opset=23)


def norm_graph(W, kind, e, t):
    nodes, inits = [W.node("Reshape", ["X", "s"], ["x3"])], [W.tensor("s", np.asarray([-1, t, e], np.int64)), W.tensor("g", np.ones(e, np.float32))]
    if kind == "rms":
        nodes.append(W.node("RMSNormalization", ["x3", "g"], ["out"], [W.attr_i("axis", -1), W.attr_f("epsilon", 1e-5)], name="rms"))
    else:
        inits.append(W.tensor("b", np.zeros(e, np.float32)))
        nodes.append(W.node("LayerNormalization", ["x3", "g", "b"], ["out"], [W.attr_i("axis", -1), W.attr_f("epsilon", 1e-5)], name="ln"))
    return W.model("norm", nodes, inits, [W.value_info("X", ["N", t * e])], [W.value_info("out", ["N", t, e])], opset=23)


def child(cases, tag):
    from infera_amd import capi, onnx_writer as W

    torch = None
    if "5" in cases:  # torch's ROCm runtime first (tools/transformer_time.py)
        import torch
        torch.cuda.is_available() and torch.zeros(1).cuda()
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)

    def timed(name, blob, x, out_per_row):
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
        d_in, d_out = capi.DeviceBuffer(dev, x.nbytes), capi.DeviceBuffer(dev, ROWS * out_per_row * 4)
        d_in.upload(x)
        capi.predict_device(name, d_in, ROWS, x.shape[1], d_out)
        ms = sorted(capi.time_predict_device(name, d_in, ROWS, x.shape[1], d_out, 3) / 3 for _ in range(REPS))
        kinds = "+".join(s["kind"] for s in capi.get_plan(name)["plan"]["steps"])
        capi.unload_model(name)
        del d_in, d_out
        return ms[len(ms) // 2], ms[0], ms[-1], kinds

    def line(what, r, extra=""):
        print(f"{tag:<14} {what:<58} {ROWS} rows: median {r[0]:8.3f} ms (min {r[1]:8.3f}, max {r[2]:8.3f}, n={REPS}) [{r[3]}]{extra}", flush=True)

    shape = f"T={T} h={HQ} dh={DH}"
    rng = np.random.default_rng(E)
    x = rng.random((ROWS, T * 3 * E), dtype=np.float32) * 2 - 1 if set(cases) & set("1235") else None
    if "1" in cases:
        line(f"(1) pattern form, unmasked, {shape}", timed("p_plain", pattern_graph(W, False), x, T * E))
    if "2" in cases:
        line(f"(2) pattern form, constant causal mask, {shape}", timed("p_causal", pattern_graph(W, True), x, T * E))
    if "3" in cases:
        line(f"(2) operator, is_causal, {shape}", timed("o_causal", op_graph(W, HQ, True), x, T * E))
        for hkv in (8, 2, 1):
            w = T * (E + 2 * hkv * DH)
            for causal in (False, True):
                r = timed(f"o_kv{hkv}_{int(causal)}", op_graph(W, hkv, causal), np.ascontiguousarray(x[:, :w]), T * E)
                line(f"(3) operator, hkv={hkv}{', is_causal' if causal else ''}, {shape}", r)
    if "5" in cases:
        if not torch.cuda.is_available():
            print(f"{tag:<14} (5) torch-ROCm scaled_dot_product_attention: NOT MEASURED, this torch build ({torch.__version__}) reports no usable GPU here", flush=True)
        else:
            qkv = torch.from_numpy(x.reshape(ROWS, T, 3, HQ, DH)).cuda()
            q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3).contiguous() for j in range(3))
            del qkv
            F_ = torch.nn.functional
            for _ in range(3):
                F_.scaled_dot_product_attention(q, k, v, is_causal=True)
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    F_.scaled_dot_product_attention(q, k, v, is_causal=True)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) / 3)
            ts.sort()
            line(f"(5) torch-ROCm f32 SDPA, is_causal, {shape}", (ts[len(ts) // 2], ts[0], ts[-1], "[N,h,T,dh] resident"))
            del q, k, v
            torch.cuda.empty_cache()
    del x
    if "4" in cases:
        for e, t in ((64, 128), (768, 16)):
            xn = np.random.default_rng(e).random((ROWS, t * e), dtype=np.float32) * 2 - 1
            for kind in ("ln", "rms"):
                r = timed(f"{kind}{e}", norm_graph(W, kind, e, t), xn, t * e)
                line(f"(4) {'RmsNorm' if kind == 'rms' else 'LayerNorm'}, E={e}, {t} vectors per row", r, f"; {ROWS * t * e * 8 / r[0] / 1e9:6.2f} TB/s of 8 bytes per element")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="ab/parent/libinfera.so")
    ap.add_argument("--child", default="")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tag)

    def leg(cases, tag, **env):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cases, "--tag", tag], env=dict(os.environ, **env), timeout=600)
        if p.returncode != 0:  # (a fault or a hang in one leg: nothing more is started on the GPU)
            sys.exit(f"leg {tag} ended with status {p.returncode}")

    if os.path.exists(a.parent_lib):
        for i in range(3):
            leg("12", f"parent run {i + 1}", INFERA_LIB_PATH=os.path.abspath(a.parent_lib))
            leg("12", f"this run {i + 1}")
    else:
        print(f"(1), (2) on the parent commit: NOT MEASURED, {a.parent_lib} is missing (build the parent commit's libinfera.so there)", flush=True)
        for i in range(3):
            leg("12", f"this run {i + 1}")
    leg("345", "this")


if __name__ == "__main__":
    main()
