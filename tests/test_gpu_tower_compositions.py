"""Every tower pass -- keds_tower_forward, keds_vit_run, keds_vit_run_tokens, keds_text_run_ex, keds_text_run_packed,
keds_text_run_tokens -- against its chain of kernels, bit for bit (tests/tower_check.py: the chain as data), and every link of the chain
within its kernel's existing bound on the link's actual inputs.

One side runs the public pass once, on a workspace of exactly the reported bytes inside a sentinel buffer, prefilled with 0xFF bytes and
again with zeros.  The other side runs the plan's steps one public call at a time on test-owned buffers, one tensor per named buffer:
16-bit and fp32 buffers filled with NaN, byte buffers with the e4m3 NaN byte 0x7F, statistics with 0xFF bytes, guard rows behind every
buffer.  The chain registers KEDS_SPLITK_BYTES of split-K scratch so that its GEMMs are planned as the tower's are, and after each link
holds what keds_gemm_last_launch / keds_gemm_mxfp8_last_launch / keds_attention_last_launch recorded to the planner's answer for that
shape.  Both side-lane settings run.  Tower and chain each run once per case: a mismatch is a finding to be read from the code.

Also here, because no per-kernel test reaches them: keds_im2col_f32 by bits, and the fp32 read-out's L2 normalisation (it has no entry of
its own) per element against row_check.l2_expected of the same pass's un-normalised output."""
import ctypes as C

import pytest
import torch

import keds_amd
from keds_amd import _lib
from oracle import keds_oracle as O
from tests import attention_check as ac
from tests import gemm_check as gc
from tests import mx_check as mx
from tests import row_check as rc
from tests import tower_check as tc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 8                                            # guard rows behind every chain buffer
NAN = float("nan")
TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
PREC = {"bf16": "bf16", "unfolded": "bf16", "fp16": "fp16", "fp8": "fp8", "f32": "fp32", "x3": "fp32x3"}
FLAGS = {"bf16": (0, 0, 0), "unfolded": (0, 0, 0), "fp16": (0, 0, 1), "fp8": (1, 0, 0), "f32": (0, 1, 0), "x3": (0, 2, 0)}   # fp8, f32, f16
E_WORKSPACE = -3
SCALE_OF = {"xq": "xs", "aq": "as", "hq": "hs"}
P = _lib.ptr
OUT_TYPE = {0: torch.bfloat16, 1: torch.float32, 2: torch.float16}
OUT_NAME = {0: "bf16", 1: "fp32", 2: "fp16"}


def _done(rc_, what):
    """a failed launch or a device fault: nothing more of this session may run on the card"""
    try:
        _lib.check(rc_, what)
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


_MODELS = {}


def _blocks(flow, width, layers, res=56):
    """the engine's own packed block parameters of a synthetic tower (unfolded: a copy with the folded pointers nulled)"""
    key = (PREC[flow], width, layers, res)
    if key not in _MODELS:
        sd = O.synth_clip_state_dict(embed_dim=128, image_resolution=res, vision_layers=layers, vision_width=width, vision_patch_size=14,
                                     context_length=77, vocab_size=512, transformer_width=256 if width == 256 else 128,
                                     transformer_layers=layers if width == 256 else 1, seed=21)
        m = keds_amd.build_model(dict(sd), fp16=False).cuda()
        m.set_precision(PREC[flow])
        _MODELS[key] = (m, m._engine())
    eng = _MODELS[key][1]
    src = eng.vit.tower.blocks
    if flow != "unfolded":
        return src
    own = (_lib.BlockParams * layers)()
    for i in range(layers):
        C.memmove(C.byref(own[i]), C.byref(src[i]), C.sizeof(_lib.BlockParams))
        own[i].qkv_wf = own[i].fc_wf = own[i].qkv_bc = own[i].fc_bc = None
    return own


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Chain:
    """the plan's steps, one public call each, on buffers of its own"""

    def __init__(self, plan, blocks, x=None, front=None, inputs=None, out_type=1):
        """front: name -> device pointer of the pass's own weights; inputs: img / tokens / rows / seq_off / img_tokens (device tensors);
        out_type: the type of taps / tokens (0 bf16, 1 fp32, 2 fp16)"""
        self.p, self.blocks, self.lib = plan, blocks, _lib.load()
        self.front_t, self.inputs, self.out_type = front or {}, inputs or {}, out_type
        self.front = {k: v.data_ptr() for k, v in self.front_t.items()}
        self.links, self.eng = None, None                # links: a dict to hold every link to its kernel's bound (worst ratios by kind)
        self.bufs, self.fill = {}, {}
        if "tokens_out" in plan.buffers:
            r, c, _ = plan.buffers["tokens_out"]
            plan.buffers["tokens_out"] = (r, c, OUT_NAME[out_type])
        for name, (r, c, t) in plan.buffers.items():
            if name == "splitk":
                continue
            if t in TYPES:
                b = torch.full((r + G, c), NAN, dtype=TYPES[t], device=DEV)
            elif t == "pair":
                b = torch.full((2 * r + G, c), NAN, dtype=torch.float16, device=DEV)          # planes [2][r][c]
            elif t == "stat":
                b = torch.full((r + G, 2), -1, dtype=torch.int64, device=DEV)
            else:
                b = torch.full((r * c + 256,), 0x7F, dtype=torch.uint8, device=DEV)
            self.bufs[name] = b
        if x is not None:
            self.bufs["x"][:x.shape[0]] = x
        if plan.find(op="tap"):
            self.taps = torch.full((plan.layers * plan.M + G, plan.w), NAN, dtype=OUT_TYPE[out_type], device=DEV)
            self.tokens = torch.full((plan.M + G, plan.w), NAN, dtype=OUT_TYPE[out_type], device=DEV)
        self.records = {"gemm_splits_max": 1, "attn_forms": set(), "attn_flags": 0}

    def guards_intact(self):
        bad = []
        for name, (r, c, t) in self.p.buffers.items():
            if name == "splitk":
                continue
            b = self.bufs[name]
            if t in TYPES or t == "pair":
                ok = bool(torch.isnan(b[(2 * r if t == "pair" else r):]).all())
            elif t == "stat":
                ok = bool((b[r:] == -1).all())
            else:
                ok = bool((b[r * c:] == 0x7F).all())
            if not ok:
                bad.append(name)
        return bad

    def addr(self, ref):
        name, r0, _ = ref
        r, c, t = self.p.buffers[name]
        return self.bufs[name].data_ptr() + r0 * c * (2 if t == "pair" else tc.ESIZE[t])

    def stat(self, name, r0):
        return None if name is None else self.bufs[name].data_ptr() + r0 * 16

    def ld(self, ref):
        return self.p.buffers[ref[0]][1] * ref[2]

    def run(self):
        # the package's own registration for direct GEMM calls: keds_gemm_set_workspace with 8 MiB = KEDS_SPLITK_BYTES, what a
        # tower's split-K scope carves for itself
        _lib.ensure_gemm_workspace()
        assert _lib._gemm_ws[torch.cuda.current_device()].numel() == tc.SPLITK_BYTES
        for s in self.p.steps:
            pre = self._before(s) if self.links is not None else None
            getattr(self, "_" + s["op"])(s)
            if pre is not None:
                self._after(s, pre)
        torch.cuda.synchronize()

    # -- every link within its kernel's bar (the existing checks, their existing constants) ------------------------------------------------
    def weight(self, ptr, shape, dtype):
        """a tensor over the engine's own packed bytes at `ptr`"""
        n = dtype.itemsize
        for d in shape:
            n *= d
        for b in self.eng.keep:
            if isinstance(b, torch.Tensor) and b.dtype == torch.uint8 and b.data_ptr() <= ptr and ptr + n <= b.data_ptr() + b.numel():
                o = ptr - b.data_ptr()
                return b[o:o + n].view(dtype).reshape(shape)
        raise LookupError("pointer outside the engine's packed blocks")

    def rows_of(self, ref, n, dtype=None, plane=0):
        name, r0, rs = ref
        t = self.bufs[name][plane + r0:][::rs][:n]
        return (t.view(dtype) if dtype is not None and t.dtype != dtype else t).clone()

    def _code16(self, s):
        """the 16-bit kernels' epilogue id of a plan step: (bf16 operands, the fp16 operating point)"""
        return {"ln_bias": (10, 16), "ln_qgelu": (11, 17), "resid_stats": (9, 18), "resid": (3, 19), "qgelu": (1, 20), "bias": (0, 0)}[s["epi"]][self.p.eff == "fp16"]

    def mx_rows(self, name, n, cols):
        """(bytes [n, cols], block exponents [n, cols / 32]) of an MXFP8 buffer of n rows (its scale array padded to n rows)"""
        q = self.bufs[name][:n * cols].view(n, cols).clone()
        sb = self.bufs[SCALE_OF[name]][:n * cols // 32].view(cols // 128, n, 4)
        return q, mx.unpack_scales(sb, n)

    def _before(self, s):
        if s["op"] == "gemm" and s["kern"] == "mx":
            n = s["n"]
            K = self.p.buffers[s["a"][0]][1]
            pre = {"A": self.mx_rows(s["a"][0], n, K)}
            if s["epi"] == "resid_stats":
                pre["resid"] = self.bufs["h"][:n].float()
            if s.get("st_read"):
                pre["stats"] = self.bufs[s["st_read"]][:n].clone()
            if s.get("st_add"):
                pre["st_add"] = self.bufs[s["st_add"]][:n].clone()
            return pre
        if s["op"] == "gemm" and s["kern"] != "mx" and s["layer"] is not None:
            pre = {}
            n = s["n"]
            if s["kern"] == "16":
                op, od, fam = gc.EPILOGUES[self._code16(s)]
            elif s["kern"] == "f32":
                op, od, fam = gc.F32, gc.F32, s["epi"]
            else:
                op, od, fam = gc.HF, gc.F32, s["epi"]
            if s["kern"] == "x3":
                pl = tc.pad256(self.p.B) if s.get("tail") else self.p.buffers[s["a"][0]][0]
                pre["A"] = (self.rows_of(s["a"], n), self.rows_of(s["a"], n, plane=pl))
            else:
                pre["A"] = self.rows_of(s["a"], n, op)
            if s["epi"].startswith("resid"):
                pre["resid"] = self.rows_of(s["out"], n, od).float()
            if s.get("st_read"):
                pre["stats"] = self.bufs[s["st_read"]][s["st_r0"]:s["st_r0"] + n].clone()
            if s.get("st_add"):
                pre["st_add"] = self.bufs[s["st_add"]][s["st_r0"]:s["st_r0"] + n].clone()
            return pre
        if s["op"] == "ln":
            return {"x": self.rows_of(s["src"], s["n"])}
        if s["op"] in ("attn", "patch", "cast", "stats_cast", "quant", "gather", "im2col", "cls"):
            return {}
        if s["op"] == "embed":
            return {"x": self.bufs["x"].clone()}
        return None

    def _note(self, key, fails, worst):
        key = f"{self.p.flow}.{key}"
        self.links[key] = max(self.links.get(key, 0.0), worst)
        assert not fails, f"{key}: " + "; ".join(str(f) for f in fails)

    def _after(self, s, pre):
        p, n, w = self.p, s.get("n"), self.p.w
        if s["op"] == "gemm":
            k = self.blocks[s["layer"]]
            N, K = {"qkv": (3 * w, w), "out": (w, w), "fc": (4 * w, w), "proj": (w, 4 * w)}[s["w"]]
            if s["kern"] == "x3":
                code = {"bias": 13, "qgelu": 15, "resid": 14}[s["epi"]]
                wp = self.weight(getattr(k, s["w"] + "_w"), (2, N, K), gc.HF)
                bias = self.weight(getattr(k, s["w"] + "_b"), (N,), gc.F32)
                case = gc.X3Case.from_operands(pre["A"][0], pre["A"][1], wp[0], wp[1], k.x3_exp[("qkv", "out", "fc", "proj").index(s["w"])], bias,
                                               pre.get("resid"))
                exp = gc.expected(case, code)
                if code == 15:
                    pl = tc.pad256(p.B) if s.get("tail") else p.buffers["hid"][0]
                    got = self.rows_of(s["out"], n).double() + self.rows_of(s["out"], n, plane=pl).double()
                else:
                    got = self.rows_of(s["out"], n)
                f = gc.check(got, exp, f"x3 {s['w']} block {s['layer']}")
                self._note("gemm_x3." + s["epi"], [f] if f else [], f.worst)
                return
            if s["kern"] == "mx":
                epi = {"ln_bias": 1, "ln_qgelu": 2, "resid_stats": 4}[s["epi"]]
                ln = s["epi"].startswith("ln")
                wq = self.weight(getattr(k, s["w"] + "_q8"), (N, K), torch.uint8)
                ws = self.weight(getattr(k, s["w"] + "_s8"), (K // 128, N, 4), torch.uint8)
                b = self.weight(getattr(k, s["w"] + ("_bc8" if ln else "_b")), (2 * N if ln else N,), gc.F32)
                case = mx.MxCase.from_operands(pre["A"][0], pre["A"][1], wq, mx.unpack_scales(ws, N), b[:N], pre.get("resid"), pre.get("stats"),
                                               b[N:] if ln else None)
                res = {}
                if epi != 2:
                    res["out"] = self.rows_of(s["out"], n)
                qname = s["out"][0] if epi == 2 else s.get("qout")
                if qname:
                    res["q"], res["qexp"] = self.mx_rows(qname, n, N)
                if s.get("st_add"):
                    res["stats"] = self.bufs[s["st_add"]][:n] - pre["st_add"]
                fails, worst = mx.model_failures(case, epi, res)
                self._note("gemm_mx." + s["epi"], fails, worst)
                return
            if s["kern"] == "f32":
                code = {"bias": 0, "qgelu": 1, "resid": 2}[s["epi"]]
                W = self.weight(getattr(k, s["w"] + "_w"), (N, K), gc.F32)
                bias = self.weight(getattr(k, s["w"] + "_b"), (N,), gc.F32)
                case = gc.Case.from_operands(pre["A"], W, bias, pre.get("resid"))
                f = gc.check(self.rows_of(s["out"], n), gc.expected(case, code), f"f32 {s['w']} block {s['layer']}")
                self._note("gemm_f32." + s["epi"], [f] if f else [], f.worst)
                return
            code = self._code16(s)
            op, od, fam = gc.EPILOGUES[code]
            folded = s["epi"].startswith("ln")
            W = self.weight(getattr(k, s["w"] + ("_wf" if folded else "_w")), (N, K), op)
            b = self.weight(getattr(k, s["w"] + ("_bc" if folded else "_b")), (2 * N if folded else N,), gc.F32)
            case = gc.Case.from_operands(pre["A"], W, b[:N], pre.get("resid"), pre.get("stats"), b[N:] if folded else None)
            exp = gc.expected(case, code)
            out = self.rows_of(s["out"], n, od)
            fs = [gc.check(out, exp, f"{gc.NAMES[code]} {s['w']} block {s['layer']}")]
            if s.get("st_add"):                          # the statistics it added: of the fp32 sums whose fp16 roundings it stored
                added = self.bufs[s["st_add"]][s["st_r0"]:s["st_r0"] + n] - pre["st_add"]
                o64 = out.double()
                fs.append(gc.check_stats(added, o64, gc.UNIT[od] * (1 + 2 * gc.UNIT[od]) * o64.abs() + gc.TINY[od], False, f"{s['w']} block {s['layer']}"))
            if s.get("st_clear"):
                assert bool((self.bufs[s["st_clear"]][s["st_r0"]:s["st_r0"] + n] == 0).all()), "the consumer did not clear the next producer's rows"
            self._note("gemm16." + s["epi"], [f for f in fs if f], max(f.worst for f in fs))
        elif s["op"] == "cast":                          # exact links: by bits against torch
            f = rc.bits_failures(self.rows_of(s["dst"], n), rc.cast_ref(self.rows_of(s["src"], n), gc.F32), "stream back to fp32")
            self._note("exact.cast", [f] if f else [], f.worst)
        elif s["op"] == "gather":
            src, rows = self.bufs[s["src"]], self.inputs["rows"].long()
            idx = rows if s["glob"] else torch.arange(n, device=DEV) * s["S"] + rows
            ok = (rows >= 0) & (rows < s["bound"])
            dst = self.bufs[s["dst"]][:n]
            want = torch.where(ok[:, None], src[torch.where(ok, idx, 0)].to(dst.dtype), torch.full_like(dst, NAN))
            f = rc.bits_failures(dst, want, "read-out rows gathered")
            self._note("exact.gather", [f] if f else [], f.worst)
        elif s["op"] == "im2col":
            rows = p.B * (s["res"] // s["patch"]) ** 2
            f = rc.bits_failures(self.bufs["col"][:rows], rc.im2col_ref(self.inputs["img"], s["patch"], s["kpad"], self.bufs["col"].dtype), "im2col")
            self._note("exact.im2col", [f] if f else [], f.worst)
        elif s["op"] == "cls":
            t = self.eng.keep[0]
            f = rc.bits_failures(self.bufs["x"][:p.M:p.S], (t["class_emb"] + t["pos_emb"][0]).expand(p.B, w).contiguous(), "cls rows")
            self._note("exact.cls_rows", [f] if f else [], f.worst)
        elif s["op"] == "embed":
            tt = next(d for d in self.eng.keep if isinstance(d, dict) and "token_emb" in d)
            nt, c0 = s["splice"] if s["splice"] else (0, 0)
            img = self.inputs["img_tokens"].cpu() if s["splice"] else None
            off = self.inputs["seq_off"].cpu() if s["packed"] else None
            want = rc.embed_ref(self.inputs["tokens"].cpu(), tt["token_emb"].cpu(), tt["pos_emb"].cpu(), img, nt, c0, pre["x"].cpu(), p.B, s["L"], s["Lx"], w, off)
            f = rc.bits_failures(self.bufs["x"].cpu(), want, "embed_tokens")
            self._note("exact.embed_tokens", [f] if f else [], f.worst)
        elif s["op"] == "stats_cast":
            x = self.bufs["x"][:n]
            fs = [rc.bits_failures(self.bufs["h"][:n], rc.cast_ref(x, gc.HF), "fp16 copy of the stream"),
                  gc.check_stats(self.bufs[s["st"]][:n], x.double(), None, False, "rowstats_cast")]
            self._note("exact.stats_cast", [f for f in fs if f], max(f.worst for f in fs))
        elif s["op"] == "quant":
            q, qexp = self.mx_rows("xq", n, w)
            fs = mx.check_mx_equal(q, qexp, self.bufs["x"][:n].double(), "MXFP8 copy of the stream")
            self._note("exact.quantise", [f for f in fs if f], max(f.worst for f in fs))
        elif s["op"] == "ln" and s["layer"] is None:     # ln_pre in place, ln_final over every column
            ref, e = rc.ln_reference(pre["x"], self.front_t[s["g"] + "_g"], self.front_t[s["g"] + "_b"])
            od = TYPES[p.buffers[s["dst"][0]][2]]
            f = gc.check(self.rows_of(s["dst"], n).double(), rc.Expected(ref, e, od, False), s["g"])
            self._note("layernorm", [f] if f else [], f.worst)
        elif s["op"] == "patch":                         # out = acc + pos[1 + m % G]: the arithmetic of a residual epilogue on pos rows
            G_, M_ = s["G"], p.B * s["G"]
            f32 = p.flow in ("f32", "x3")
            case = gc.Case.from_operands(self.bufs["col"][:M_].clone(), self.front_t["conv_w"], None, self.front_t["vit_pos"][1:].repeat(p.B, 1))
            got = self.bufs["x"][:p.M].view(p.B, p.S, w)[:, 1:].reshape(M_, w)
            f = gc.check(got, gc.expected(case, 2 if f32 else 19 if p.flow == "fp16" else 3), "patch embedding")
            self._note("gemm_f32.patch" if f32 else "gemm16.patch", [f] if f else [], f.worst)
        elif s["op"] == "ln":
            k = self.blocks[s["layer"]]
            g, b = (self.weight(getattr(k, s["g"] + t), (w,), gc.F32) for t in ("_g", "_b"))
            ref, e = rc.ln_reference(pre["x"], g, b)
            if p.eff == "x3":
                pl = tc.pad256(p.B) if s.get("tail") else p.buffers["ln"][0]
                got = self.rows_of(s["dst"], n).double() + self.rows_of(s["dst"], n, plane=pl).double()
                exp = rc.Expected(ref, e, gc.HF, False, pair=True)
            else:
                od = gc.F32 if s["dst"][0] == "ln" else gc.HF if p.eff == "fp16" else gc.BF
                got = self.rows_of(s["dst"], n, od).double()
                exp = rc.Expected(ref, e, od, False)
            f = gc.check(got, exp, f"{s['g']} block {s['layer']}")
            self._note("layernorm", [f] if f else [], f.worst)
        elif s["op"] == "attn":
            kern = tc._kern(p.eff)
            lens = s["S"] if s["off"] is None else [s["off"][b + 1] - s["off"][b] for b in range(s["B"])]
            M = s["B"] * s["S"] if s["off"] is None else s["off"][-1]
            case = ac.Case(self.bufs[s["qkv"]][:M].clone(), s["B"], lens, p.heads, s["causal"])
            ql = s["q_limit"] if s["q_limit"] < s["S"] else None
            if kern == "16" and s["q8_rows"]:
                # rows < q8_rows left as MXFP8 (held by the attention bar's own MXFP8 cases); the remainder rows went to `att` as bf16
                rows = torch.arange(M, device=DEV) >= s["q8_rows"]
                ratio = (self.bufs[s["out"]][:M].double() - case.o).abs() / case.bound()
                f = ac._collect(torch.where(rows[:, None], ratio, torch.zeros_like(ratio)), case, rows, 1.0)
                self._note("attention.remainder_rows_beside_mxfp8", [str(f)] if len(f) else [], f.worst)
                return
            if kern == "16":
                f = ac.check(self.bufs[s["out"]][:M], case, ql)
            elif s["out"] == "ln":                       # the planes of the split-fp16 form
                pl = p.buffers["ln"][0]
                f = ac.check_f32(self.bufs["ln"][:M].double() + self.bufs["ln"][pl:pl + M].double(), case, ql, abs_floor=2.0 ** -24)
            else:
                f = ac.check_f32(self.bufs[s["out"]][:M], case, ql, abs_floor=2.0 ** -25 if kern == "x3" else 0.0)
            self._note("attention", [str(f)] if len(f) else [], f.worst / f.limit)

    # -- links ----------------------------------------------------------------------------------------------------------------------
    def _rec_gemm(self, epi, M, N, K, lda, ldc, what):
        got, want = (C.c_int * 8)(), (C.c_int * 8)()
        _lib.check(self.lib.keds_gemm_last_launch(got), "keds_gemm_last_launch")
        _lib.check(self.lib.keds_gemm_plan_query(epi, M, N, K, lda, ldc, _cus(), tc.SPLITK_BYTES, 0, want), "keds_gemm_plan_query")
        assert list(got) == list(want), f"{what}: launched {list(got)}, planned {list(want)}"
        self.records["gemm_splits_max"] = max(self.records["gemm_splits_max"], got[4], got[5])

    def _gemm(self, s):
        lib, st, p = self.lib, _lib.stream(), self.p
        k = self.blocks[s["layer"]]
        n, w = s["n"], p.w
        N, K = {"qkv": (3 * w, w), "out": (w, w), "fc": (4 * w, w), "proj": (w, 4 * w)}[s["w"]]
        a, o = self.addr(s["a"]), self.addr(s["out"])
        lda, ldc = self.ld(s["a"]), self.ld(s["out"])
        what = f"{p.flow} block {s['layer']} {s['w']} rows [{s['st_r0']}, +{n})"
        if s["kern"] == "16":
            epi = self._code16(s)
            folded = s["epi"].startswith("ln")
            W = getattr(k, s["w"] + ("_wf" if folded else "_w"))
            bias = getattr(k, s["w"] + ("_bc" if folded else "_b"))
            aux = self.stat(s.get("st_read") or s.get("st_add"), s["st_r0"])
            aux2 = self.stat(s.get("st_clear"), s["st_r0"])
            _done(lib.keds_gemm_bt_ex2(a, lda, W, bias, o, ldc, n, N, K, epi, aux, 0, aux2, st), what)
            self._rec_gemm(epi, n, N, K, lda, ldc, what)
        elif s["kern"] == "mx":
            epi = {"ln_bias": 1, "ln_qgelu": 2, "resid_stats": 4}[s["epi"]]
            Wq, Ws = getattr(k, s["w"] + "_q8"), getattr(k, s["w"] + "_s8")
            bias = getattr(k, s["w"] + "_bc8") if s["epi"].startswith("ln") else getattr(k, s["w"] + "_b")
            As = self.bufs[SCALE_OF[s["a"][0]]].data_ptr()
            aux = self.stat(s.get("st_read") or s.get("st_add"), 0)
            aux2 = self.stat(s.get("st_clear"), 0)
            qname = s["out"][0] if s["epi"] == "ln_qgelu" else s.get("qout")
            qo = self.bufs[qname].data_ptr() if qname else None
            qs = self.bufs[SCALE_OF[qname]].data_ptr() if qname else None
            out = None if s["epi"] == "ln_qgelu" else o
            assert s["st_r0"] == 0 and n % 256 == 0
            _done(lib.keds_gemm_mxfp8_ex(a, As, n, Wq, Ws, N, bias, out, n, N, K, epi, aux, aux2, qo, qs, n if qname else 0, st), what)
            got, want = (C.c_int * 4)(), (C.c_int * 4)()
            _lib.check(lib.keds_gemm_mxfp8_last_launch(got), "keds_gemm_mxfp8_last_launch")
            _lib.check(lib.keds_gemm_mxfp8_plan_query(epi, n, N, K, _cus(), want), "keds_gemm_mxfp8_plan_query")
            assert list(got) == list(want), f"{what}: launched {list(got)}, planned {list(want)}"
        elif s["kern"] == "f32":
            epi = {"bias": 0, "qgelu": 1, "resid": 2}[s["epi"]]
            _done(lib.keds_gemm_f32(a, lda, getattr(k, s["w"] + "_w"), getattr(k, s["w"] + "_b"), o, ldc, n, N, K, epi, None, 0, st), what)
        else:                                            # split fp16 operands: planes of A, of W and (c_fc) of the output
            epi = {"bias": 13, "qgelu": 15, "resid": 14}[s["epi"]]
            rows_a = tc.pad256(p.B) if s.get("tail") else p.buffers[s["a"][0]][0]
            a_plane = rows_a * K
            o_plane = (tc.pad256(p.B) if s.get("tail") else p.buffers["hid"][0]) * N if epi == 15 else 0
            wi = ("qkv", "out", "fc", "proj").index(s["w"])
            _done(lib.keds_gemm_x3(a, a_plane, lda, getattr(k, s["w"] + "_w"), N * K, getattr(k, s["w"] + "_b"), o, ldc, n, N, K, epi, o_plane,
                                   k.x3_exp[wi], st), what)
            self._rec_gemm(epi, n, N, K, lda, ldc, what)

    def _attn(self, s):
        lib, st, p = self.lib, _lib.stream(), self.p
        q, B, S, H, c, ql = self.bufs[s["qkv"]].data_ptr(), s["B"], s["S"], p.heads, int(s["causal"]), s["q_limit"]
        what = f"{p.flow} attention q_limit {ql}"
        kern = tc._kern(p.eff)
        if s["off"] is not None and kern != "16":        # packed rows of the fp32 and split-fp16 forms
            assert ql == S
            so = P(self.inputs["seq_off"])
            if kern == "f32":
                _done(lib.keds_attention_f32_packed(q, self.bufs[s["out"]].data_ptr(), B, S, so, H, c, st), what + " packed")
            elif s["out"] == "ln":
                _done(lib.keds_attention_x3_packed(q, None, self.bufs["ln"].data_ptr(), p.buffers["ln"][0] * p.w, B, S, so, H, c, None, st), what + " packed")
            else:
                _done(lib.keds_attention_x3_packed(q, self.bufs[s["out"]].data_ptr(), None, 0, B, S, so, H, c, None, st), what + " packed")
            return
        if s["off"] is not None:                         # packed rows of the 16-bit forms
            assert ql == S
            f16 = int(p.eff == "fp16")
            fn = lib.keds_attention_packed_h if f16 else lib.keds_attention_packed
            _done(fn(q, self.bufs[s["out"]].data_ptr(), B, S, P(self.inputs["seq_off"]), H, c, st), what + " packed")
            got, want = (C.c_int * 8)(), (C.c_int * 8)()
            _lib.check(lib.keds_attention_last_launch(got), "keds_attention_last_launch")
            _lib.check(lib.keds_attention_plan_query(B, S, H, c, ql, f16, 0, 1, want), "keds_attention_plan_query")
            assert list(got) == list(want), f"{what}: launched {list(got)}, planned {list(want)}"
            return
        if kern == "f32":
            _done(lib.keds_attention_f32(q, self.bufs[s["out"]].data_ptr(), B, S, H, c, ql, st), what)
            return
        if kern == "x3":
            if s["out"] == "ln":                         # the planes of the out-projection's A operand
                _done(lib.keds_attention_x3(q, None, self.bufs["ln"].data_ptr(), p.buffers["ln"][0] * p.w, B, S, H, c, ql, None, st), what)
            else:
                _done(lib.keds_attention_x3(q, self.bufs[s["out"]].data_ptr(), None, 0, B, S, H, c, ql, None, st), what)
            return
        o = self.bufs[s["out"]].data_ptr()
        f16 = int(p.eff == "fp16")
        if f16:
            _done(lib.keds_attention_h(q, o, B, S, H, c, ql, st), what)
        elif s["q8_rows"]:
            _done(lib.keds_attention_mx(q, o, B, S, H, c, ql, self.bufs["aq"].data_ptr(), self.bufs["as"].data_ptr(), s["q8_rows"], st), what)
        else:
            _done(lib.keds_attention_ex(q, o, B, S, H, c, ql, st), what)
        got, want = (C.c_int * 8)(), (C.c_int * 8)()
        _lib.check(lib.keds_attention_last_launch(got), "keds_attention_last_launch")
        _lib.check(lib.keds_attention_plan_query(B, S, H, c, ql, f16, int(s["q8_rows"] > 0), 0, want), "keds_attention_plan_query")
        assert list(got) == list(want), f"{what}: launched {list(got)}, planned {list(want)}"
        self.records["attn_forms"].add(got[0])
        self.records["attn_flags"] |= got[3]

    def _ln(self, s):
        lib, st, p = self.lib, _lib.stream(), self.p
        src, dst = self.addr(s["src"]), self.addr(s["dst"])
        if s["layer"] is None:                           # ln_pre in place, ln_final over every column: fp32 in, the buffer's type out
            code = {"fp32": 1, "bf16": 0, "fp16": 2}[p.buffers[s["dst"][0]][2]]
            _done(lib.keds_layernorm_rows(src, p.w, None, 1, self.front[s["g"] + "_g"], self.front[s["g"] + "_b"], dst, code, s["n"], p.w, st), s["g"])
            return
        k = self.blocks[s["layer"]]
        g, b = getattr(k, s["g"] + "_g"), getattr(k, s["g"] + "_b")
        what = f"{p.flow} block {s['layer']} {s['g']}"
        if p.eff == "x3":
            assert s["src"][2] == 1
            plane = (tc.pad256(p.B) if s.get("tail") else p.buffers["ln"][0]) * p.w
            _done(lib.keds_layernorm_pair(src, p.w, g, b, dst, plane, s["n"], p.w, 0, st), what)
            return
        out_type = 1 if s["dst"][0] == "ln" else 2 if p.eff == "fp16" else 0
        _done(lib.keds_layernorm_rows(src, p.w, None, s["src"][2], g, b, dst, out_type, s["n"], p.w, st), what)

    def _stats_cast(self, s):
        assert s["r0"] == 0
        _done(self.lib.keds_rowstats_cast_ex(P(self.bufs["x"]), P(self.bufs["h"]), 1, P(self.bufs[s["st"]]), s["n"], self.p.w, _lib.stream()),
              "keds_rowstats_cast_ex")

    def _quant(self, s):
        n = s["n"]
        _done(self.lib.keds_quantize_mxfp8(P(self.bufs["x"]), 0, n, self.p.w, n, P(self.bufs["xq"]), P(self.bufs["xs"]), _lib.stream()),
              "keds_quantize_mxfp8")

    def _cast(self, s):                                  # rows of the fp16 stream back to fp32
        _done(self.lib.keds_cast_rows(self.addr(s["src"]), 2, self.addr(s["dst"]), 1, s["n"], self.p.w, self.ld(s["src"]), 0, _lib.stream()),
              "keds_cast_rows")

    def _copy(self, s):
        n = s["n"]
        src = self.bufs[s["src"][0]][s["src"][1]:][::s["src"][2]][:n]
        self.bufs[s["dst"][0]][s["dst"][1]:][::s["dst"][2]][:n] = src

    def _zero(self, s):
        self.bufs[s["buf"]][s["r0"]:s["r0"] + s["n"]] = 0

    def _gather(self, s):
        t = self.p.buffers[s["src"]][2]
        mode = 2 if t == "fp32" else 1 if s["src"] == "h" else 0          # fp32 copied; the fp16 stream to fp32; 16-bit copied
        _done(self.lib.keds_gather_token_rows(P(self.bufs[s["src"]]), P(self.bufs[s["dst"]]), P(self.inputs["rows"]), s["bound"], s["n"], self.p.w,
                                              mode, int(s["glob"]), _lib.stream()), "keds_gather_token_rows")

    def _tap(self, s):
        p, es = self.p, OUT_TYPE[self.out_type].itemsize
        r0, n = s["src"][1], s["n"]
        src_type = 2 if s["src"][0] == "h" else 1
        dsts = [self.taps.data_ptr() + (s["layer"] * p.M + r0) * p.w * es]
        if s["layer"] == p.layers - 1:
            dsts.append(self.tokens.data_ptr() + r0 * p.w * es)
        for d in dsts:
            _done(self.lib.keds_cast_rows(self.addr(s["src"]), src_type, d, self.out_type, n, p.w, p.w, 0, _lib.stream()), "tap")

    def _im2col(self, s):
        p, lib = self.p, self.lib
        img, col = P(self.inputs["img"]), P(self.bufs["col"])
        if p.flow in ("f32", "x3"):
            _done(lib.keds_im2col_f32(img, col, p.B, s["res"], s["patch"], s["kpad"], _lib.stream()), "keds_im2col_f32")
        else:
            _done(lib.keds_im2col_ex(img, col, int(p.flow == "fp16"), p.B, s["res"], s["patch"], s["kpad"], _lib.stream()), "keds_im2col_ex")

    def _patch(self, s):
        p, lib, f = self.p, self.lib, self.front
        M, K = p.B * s["G"], s["kpad"]
        if p.flow in ("f32", "x3"):
            _done(lib.keds_gemm_f32(P(self.bufs["col"]), K, f["conv_w"], None, P(self.bufs["x"]), p.w, M, p.w, K, 4, f["vit_pos"], s["G"], _lib.stream()),
                  "patch embedding (f32)")
            return
        epi = 21 if p.flow == "fp16" else 5
        _done(lib.keds_gemm_bt(P(self.bufs["col"]), f["conv_w"], None, P(self.bufs["x"]), M, p.w, K, epi, f["vit_pos"], s["G"], _lib.stream()),
              "patch embedding")
        self._rec_gemm(epi, M, p.w, K, K, p.w, "patch embedding")

    def _cls(self, s):
        p, f = self.p, self.front
        _done(self.lib.keds_cls_rows(P(self.bufs["x"]), f["class_emb"], f["vit_pos"], p.B, p.S, p.w, _lib.stream()), "keds_cls_rows")

    def _embed(self, s):
        p, f, i = self.p, self.front, self.inputs
        n_tok, col0 = s["splice"] if s["splice"] else (0, 0)
        _done(self.lib.keds_embed_tokens_ex(P(i["tokens"]), f["token_emb"], f["text_pos"], P(i["img_tokens"]) if s["splice"] else None, n_tok, col0,
                                            P(self.bufs["x"]), p.B, s["L"], s["Lx"], p.w, P(i["seq_off"]) if s["packed"] else None, _lib.stream()),
              "keds_embed_tokens_ex")

    def _readout(self, s):
        """LayerNorm of the read-out rows + projection; the L2 normalisation of the 16-bit flows has an entry, the fp32 one has none"""
        p, f, lib, st = self.p, self.front, self.lib, _lib.stream()
        if self.links is not None:
            self._readout_links(s)
        rows = P(self.inputs["rows"]) if s["rows"] else None
        g, b = f[s["g"] + "_g"], f[s["g"] + "_b"]
        ro, out = P(self.bufs["ro"]), P(self.bufs["out"])
        if p.flow in ("f32", "x3"):
            _done(lib.keds_layernorm_rows(P(self.bufs["x"]), p.w, rows, s["S"], g, b, ro, 1, p.B, p.w, st), "read-out LayerNorm")
            _done(lib.keds_gemm_f32(ro, p.w, f["proj_" + s["g"]], None, out, p.E, p.B, p.E, p.w, 0, None, 0, st), "read-out projection")
            assert not s["normalize"]
            return
        h = p.flow == "fp16"
        _done(lib.keds_layernorm_rows(P(self.bufs["x"]), p.w, rows, s["S"], g, b, ro, 2 if h else 0, p.B, p.w, st), "read-out LayerNorm")
        epi = 22 if h else 4
        _done(lib.keds_gemm_bt(ro, f["proj_" + s["g"]], None, out, p.B, p.E, p.w, epi, None, 0, st), "read-out projection")
        self._rec_gemm(epi, p.B, p.E, p.w, p.w, p.E, "read-out projection")
        self.out_raw = self.bufs["out"][:p.B].clone()
        self.out_norm = torch.empty_like(self.out_raw)
        _done(lib.keds_l2_normalize(P(self.out_raw), P(self.out_norm), p.B, p.E, st), "keds_l2_normalize")

    def _readout_links(self, s):
        """the read-out's LayerNorm (gathered rows) and projection per element, on a run of their own"""
        p, ft, lib, st = self.p, self.front_t, self.lib, _lib.stream()
        f32 = p.flow in ("f32", "x3")
        od = gc.F32 if f32 else gc.HF if p.flow == "fp16" else gc.BF
        rmap = self.inputs["rows"] if s["rows"] else None
        src, bad = rc.gather_sources(p.B, rmap, s["S"])
        x = self.bufs["x"][src.to(DEV)].clone()
        ro = torch.full((tc.pad256(p.B) + G, p.w), NAN, dtype=od, device=DEV)
        _done(lib.keds_layernorm_rows(P(self.bufs["x"]), p.w, P(rmap), s["S"], ft[s["g"] + "_g"].data_ptr(), ft[s["g"] + "_b"].data_ptr(), P(ro),
                                      rc.OUT_CODE[od], p.B, p.w, st), "read-out LayerNorm")
        good = ~bad.to(DEV) & torch.isfinite(x).all(1)
        ref, e = rc.ln_reference(x[good], ft[s["g"] + "_g"], ft[s["g"] + "_b"])
        fl = gc.check(ro[:p.B][good].double(), rc.Expected(ref, e, od, False), "read-out LayerNorm")
        self._note("layernorm.readout", [fl] if fl else [], fl.worst)
        assert torch.isnan(ro[:p.B][~good].float()).all()
        out = torch.full((p.B + G, p.E), NAN, device=DEV)
        proj = ft["proj_" + s["g"]]
        if f32:
            _done(lib.keds_gemm_f32(P(ro), p.w, P(proj), None, P(out), p.E, p.B, p.E, p.w, 0, None, 0, st), "read-out projection")
        else:
            _done(lib.keds_gemm_bt(P(ro), P(proj), None, P(out), p.B, p.E, p.w, 22 if p.flow == "fp16" else 4, None, 0, st), "read-out projection")
        case = gc.Case.from_operands(ro[:p.B][good].clone(), proj, None)
        fp = gc.check(out[:p.B][good], gc.expected(case, 0 if f32 else 22 if p.flow == "fp16" else 4), "read-out projection")
        self._note("gemm_f32.readout" if f32 else "gemm16.readout", [fp] if fp else [], fp.worst)

    def _split(self, s):
        _done(self.lib.keds_split_f16_pair(self.addr(s["src"]), self.p.w, s["n"], self.p.w, self.addr(s["dst"]), s["plane"], None, _lib.stream()),
              "keds_split_f16_pair")


def _run_tower(tp, x0, B, fill):
    """keds_tower_forward once on a workspace of exactly the reported bytes inside a sentinel buffer -> x after the pass"""
    lib = _lib.load()
    n = lib.keds_tower_workspace_bytes_ex(C.byref(tp), B)
    assert n > 0
    pad = 4096
    buf = torch.full((n + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = buf[pad:pad + n]
    ws.fill_(fill)
    x = x0.clone()
    short = lib.keds_tower_forward(C.byref(tp), P(x), B, ws.data_ptr(), n - 1, _lib.stream())
    torch.cuda.synchronize()
    assert short == E_WORKSPACE
    assert torch.equal(x.view(torch.int32), x0.view(torch.int32)), "a refused call touched x"
    _done(lib.keds_tower_forward(C.byref(tp), P(x), B, ws.data_ptr(), n, _lib.stream()), "keds_tower_forward")
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all()), "bytes around the workspace were written"
    return x


def _x3_splits(lib, M, w):
    """f32path's rule for the split-operand flow: the in_proj alone decides whether the remainder rows leave the main launch"""
    info = (C.c_int * 8)()
    _lib.check(lib.keds_gemm_plan_query(13, M, 3 * w, w, w, 3 * w, _cus(), tc.SPLITK_BYTES, 0, info), "keds_gemm_plan_query")
    return info[1] != 0


def _compose(flow, width, layers, B, S, tail, res=56, side_expected=None):
    """tower = chain by bits with the side lane on and off; -> the chain's records (lane on)"""
    lib = _lib.load()
    blocks = _blocks(flow, width, layers, res)
    fp8, f32, f16 = FLAGS[flow]
    heads = width // 64
    tp = _lib.TowerParams(width, layers, heads, S, 0, C.cast(blocks, C.POINTER(_lib.BlockParams)), fp8, int(tail == "cls"), f32, f16)
    M = B * S
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + S)
    x0 = torch.full((tc.pad256(M) + G, width), NAN, device=DEV)
    x0[:M] = torch.randn(M, width, generator=g).to(DEV)
    records = None
    try:
        for lane in (1, 0):
            _lib.check(lib.keds_side_lane_enable(lane), "keds_side_lane_enable")
            side = lib.keds_tower_side_rows(width, S, B, fp8)
            want = (M % 256 if fp8 and M >= 256 else 0) if side_expected is None else side_expected
            assert side == (want if lane else 0), f"keds_tower_side_rows({width}, {S}, {B}, {fp8}) = {side}"
            split = side > 0 if flow in ("bf16", "fp16") else bool(lane) and 0 < M // 256 * 256 < M and _x3_splits(lib, M, width) if flow == "x3" else False
            plan = tc.plan(flow, "tower", layers, B, S=S, tail=tail, width=width, heads=heads, causal=False, split=split)
            chain = Chain(plan, blocks, x0[:M])
            chain.run()
            xc = chain.bufs["x"]
            assert chain.guards_intact() == []
            rows = torch.tensor(plan.out_rows, device=DEV)
            assert torch.isfinite(xc[rows]).all(), "the chain's own output is not finite"
            for fill in (0xFF, 0x00):
                xt = _run_tower(tp, x0, B, fill)
                assert torch.isnan(xt[tc.pad256(M):]).all(), "rows behind the stream were written"
                assert torch.equal(xt[rows].view(torch.int32), xc[rows].view(torch.int32)), \
                    f"{flow} {tail} B={B} S={S} lane={lane} workspace prefilled {fill:#x}: the pass differs from its chain"
            if lane:
                records = chain.records
    finally:
        lib.keds_side_lane_enable(1)
    return records


# ---- tiny cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", ("all", "cls"))
@pytest.mark.parametrize("B", (1, 15, 16, 31))         # 17 rows; 255 (fp8 falls to the 16-bit kernels entirely); 256 + 16; 2 * 256 + 15
@pytest.mark.parametrize("flow", tc.FLOWS)
def test_tiny_tower_equals_its_chain(flow, B, tail):
    _compose(flow, 256, 3, B, 17, tail)


@pytest.mark.parametrize("flow", ("bf16", "fp16"))
def test_split_k_tower_equals_its_chain(flow):
    """width 512: c_proj has K = 2048 and few tiles, so the tower's split-K scope on its own scratch is in play"""
    rec = _compose(flow, 512, 3, 4, 17, "all")
    assert rec["gemm_splits_max"] > 1
    _compose(flow, 512, 3, 4, 17, "cls")


# ---- big cases: the smallest shapes at which the 16-bit flows put remainder rows on the side lane; bits only ------------------------
ATTN_FORM_GENERIC, ATTN_FORM_S257, ATTN_FLAG_STOP_EVENT = _lib.ATTN_FORM_GENERIC, _lib.ATTN_FORM_S257, _lib.ATTN_FLAG_STOP_EVENT


@pytest.mark.parametrize("tail", ("cls", "all"))
@pytest.mark.parametrize("B", (54, 55))
@pytest.mark.parametrize("flow", ("bf16", "fp16", "fp8", "x3"))
def test_vitl_rows_on_the_side_lane(flow, B, tail):
    """S = 257: B = 54 does not split, B = 55 puts 55 rows on the side lane; the 8-wave S = 257 attention records the fork itself"""
    side = B * 257 % 256 if flow == "fp8" else 55 if B == 55 else 0
    rec = _compose(flow, 1024, 2, B, 257, tail, res=224, side_expected=side if flow != "x3" else (55 if B == 55 else 0))
    if flow != "x3":
        assert ATTN_FORM_S257 in rec["attn_forms"] and rec["attn_flags"] & ATTN_FLAG_STOP_EVENT


def test_generic_attention_fork_is_a_recorded_marker():
    """S = 17 at B = 829: 13 rows on the side lane behind an attention form that does not take the stop event"""
    rec = _compose("bf16", 1024, 2, 829, 17, "all", res=224, side_expected=13)
    assert rec["attn_forms"] == {ATTN_FORM_GENERIC} and not rec["attn_flags"] & ATTN_FLAG_STOP_EVENT


# ---- two leftovers of the fp32 read-out ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("R,Pp,Kpad", [(28, 14, 592), (56, 14, 640), (32, 16, 768), (224, 14, 592)])
def test_im2col_f32_by_bits(R, Pp, Kpad, B):
    lib = _lib.load()
    g = torch.Generator().manual_seed(R * 10 + B)
    img = torch.randn(B, 3, R, R, generator=g)
    sp = rc.cast_specials(torch.float32)
    img.view(-1)[torch.randperm(img.numel(), generator=g)[:sp.numel()]] = sp       # the cast specials among the pixels
    img = img.to(DEV)
    rows = B * (R // Pp) ** 2
    buf = torch.full((rows + 2 * G, Kpad), rc.SENT, dtype=torch.float32, device=DEV)
    view = buf[G:G + rows]
    _done(lib.keds_im2col_f32(P(img), view.data_ptr(), B, R, Pp, Kpad, _lib.stream()), "keds_im2col_f32")
    got = view.clone()
    want = rc.im2col_ref(img, Pp, Kpad, torch.float32)
    fails = rc.bits_failures(got, want, f"im2col_f32 R{R} P{Pp} Kpad{Kpad} B{B}")
    assert not [f for f in [fails] if f], str(fails)
    assert bool((got[:, 3 * Pp * Pp:].view(torch.int32) == 0).all()), "the pad columns are +0"
    view.fill_(rc.SENT)
    assert bool((buf == rc.SENT).all()), "written outside the output rows"


def _f32_vit(embed_dim):
    key = ("l2", embed_dim)
    if key not in _MODELS:
        sd = O.synth_clip_state_dict(embed_dim=embed_dim, image_resolution=28, vision_layers=1, vision_width=128, vision_patch_size=14,
                                     context_length=77, vocab_size=512, transformer_width=128, transformer_layers=1, seed=5)
        m = keds_amd.build_model(dict(sd), fp16=False).cuda()
        m.set_precision("fp32")
        _MODELS[key] = (m, m._engine())
    return _MODELS[key][1]


def _vit_out(eng, vit, img, B, normalize):
    lib = _lib.load()
    n = lib.keds_vit_workspace_bytes(C.byref(vit), B)
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((B + G, vit.embed_dim), rc.SENT, dtype=torch.float32, device=DEV)
    _done(lib.keds_vit_run(C.byref(vit), P(img), B, P(out), normalize, P(ws), n, _lib.stream()), "keds_vit_run")
    assert bool((out[B:] == rc.SENT).all())
    return out[:B].clone()


@pytest.mark.parametrize("B", (1, 3, 4, 5))            # the kernel runs four rows per workgroup
@pytest.mark.parametrize("embed_dim", (128, 640))
def test_f32_readout_l2_normalisation(embed_dim, B):
    """l2norm_rows_f32_kernel through keds_vit_run in the f32 flow: the normalize = 1 output per element against row_check.l2_expected of the
    normalize = 0 output of the same pass (a lane's fma chain, the butterfly, one sqrtf, one division: no new constant)"""
    eng = _f32_vit(embed_dim)
    img = torch.randn(B, 3, 28, 28, generator=torch.Generator().manual_seed(B)).to(DEV)
    raw = _vit_out(eng, eng.vit, img, B, 0)
    got = _vit_out(eng, eng.vit, img, B, 1)
    assert torch.isfinite(raw).all()
    fails, worst = rc.norm_failures(got.cpu(), rc.l2_expected(raw.cpu()), f"f32 read-out l2 E{embed_dim} B{B}")
    report(f"tower_compositions.l2norm_f32.E{embed_dim}.B{B}", worst_ratio=worst)
    assert not fails, "\n".join(str(f) for f in fails)


def test_f32_readout_l2_of_a_zero_projection():
    """proj_t = 0: every projected row is all zero, the kernel divides 0 by sqrt(0) = 0 and the row is NaN -- as the reference's
    x / x.norm() is, and as the 16-bit read-out's normalisation gives for the same row"""
    eng = _f32_vit(128)
    B = 3
    img = torch.randn(B, 3, 28, 28, generator=torch.Generator().manual_seed(77)).to(DEV)
    zero = torch.zeros(128, 128, device=DEV)
    vit = _lib.VitParams()
    C.memmove(C.byref(vit), C.byref(eng.vit), C.sizeof(_lib.VitParams))
    vit.proj_t = zero.data_ptr()
    assert bool((_vit_out(eng, vit, img, B, 0) == 0).all())
    assert torch.isnan(_vit_out(eng, vit, img, B, 1)).all()
    eng16 = _engine("bf16")
    vit16 = _lib.VitParams()
    C.memmove(C.byref(vit16), C.byref(eng16.vit), C.sizeof(_lib.VitParams))
    z16 = torch.zeros(128, 256, dtype=torch.bfloat16, device=DEV)
    vit16.proj_t = z16.data_ptr()
    img16 = torch.randn(B, 3, 56, 56, generator=torch.Generator().manual_seed(78)).to(DEV)
    assert torch.isnan(_vit_out(eng16, vit16, img16, B, 1)).all()


# ---- whole passes: keds_vit_run, keds_vit_run_tokens, keds_text_run_ex, keds_text_run_packed, keds_text_run_tokens -------------------
W, LAYERS, HEADS, E, L, VOCAB = 256, 3, 4, 128, 77, 512


def _engine(flow, width=W, layers=LAYERS, res=56):
    _blocks(flow, width, layers, res)
    return _MODELS[(PREC[flow], width, layers, res)][1]


def _front(eng):
    t = eng.keep[0]
    tt = next(d for d in eng.keep if isinstance(d, dict) and "token_emb" in d)
    f = {k: t[k] for k in ("conv_w", "class_emb", "ln_pre_g", "ln_pre_b", "ln_post_g", "ln_post_b")}
    f.update(vit_pos=t["pos_emb"], proj_ln_post=t["proj_t"], token_emb=tt["token_emb"], text_pos=tt["pos_emb"], ln_final_g=tt["ln_final_g"],
             ln_final_b=tt["ln_final_b"], proj_ln_final=tt["proj_t"])
    return f


def _params(flow, which, cls_only=True, **geometry):
    """-> (a copy of the engine's VitParams / TextParams, the block array the chain uses, what keeps both alive)"""
    eng = _engine(flow, **geometry)
    src = eng.vit if which == "vit" else eng.text
    par = type(src)()
    C.memmove(C.byref(par), C.byref(src), C.sizeof(type(src)))
    blocks = src.tower.blocks
    if flow == "unfolded":
        blocks = (_lib.BlockParams * LAYERS)()
        for i in range(LAYERS):
            C.memmove(C.byref(blocks[i]), C.byref(src.tower.blocks[i]), C.sizeof(_lib.BlockParams))
            blocks[i].qkv_wf = blocks[i].fc_wf = blocks[i].qkv_bc = blocks[i].fc_bc = None
        par.tower.blocks = C.cast(blocks, C.POINTER(_lib.BlockParams))
    if which == "vit":
        par.tower.last_cls_only = int(cls_only)
    return par, blocks, eng


def _in_sentinel(nbytes, fill, call, outs):
    """`call(ws pointer, bytes)` once with one byte too few (KEDS_E_WORKSPACE, outputs untouched), once on exactly `nbytes` inside a
    sentinel buffer prefilled with `fill` -> the workspace view"""
    pad = 4096
    buf = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = buf[pad:pad + nbytes]
    ws.fill_(fill)
    before = [o.clone() for o in outs]
    short = call(ws.data_ptr(), nbytes - 1)
    torch.cuda.synchronize()
    assert short == E_WORKSPACE
    assert all(_same(o, b) for o, b in zip(outs, before)), "a refused call touched an output"
    _done(call(ws.data_ptr(), nbytes), "pass")
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + nbytes:] == 0xA5).all()), "bytes around the workspace were written"
    return ws


def _same(a, b):
    """equal bits; a NaN row of one is a NaN row of the other"""
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    eq = a.contiguous().view(it) == b.contiguous().view(it)
    if a.is_floating_point():
        eq = eq | (torch.isnan(a) & torch.isnan(b))
    return bool(eq.all())


def _lanes(flow):
    """both side-lane settings where the flow can have a remainder span at width 256 (the MXFP8 tower; the split-operand flow, whose
    in_proj alone decides), else the default"""
    return (1, 0) if flow in ("fp8", "x3") else (1,)


def _pass_split(lib, flow, S, B, lane):
    """asserts keds_tower_side_rows for the shape -> does the plan carry the remainder rows as a span of their own?"""
    M = B * S
    side = lib.keds_tower_side_rows(W, S, B, int(flow == "fp8"))
    assert side == (M % 256 if flow == "fp8" and lane and M >= 256 else 0)       # width 256: the 16-bit flows never split
    return flow == "x3" and bool(lane) and 0 < M // 256 * 256 < M and _x3_splits(lib, M, W)


def _l2_held(got, raw, what):
    """normalize = 1 of the fp32 flows (no entry of its own: no chain link) per element against row_check.l2_expected of the raw rows"""
    fails, worst = rc.norm_failures(got.cpu(), rc.l2_expected(raw.cpu()), what)
    report("tower_compositions.l2norm_f32." + what.replace(" ", "_"), worst_ratio=worst)
    assert not fails, "\n".join(str(f) for f in fails)


def _out(B):
    return torch.full((B + G, E), rc.SENT, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("cls_only", (1, 0))
@pytest.mark.parametrize("B", (1, 15, 16, 31))
@pytest.mark.parametrize("flow", tc.FLOWS)
def test_vit_run_equals_its_chain(flow, B, cls_only):
    lib = _lib.load()
    par, blocks, eng = _params(flow, "vit", bool(cls_only))
    img = torch.randn(B, 3, 56, 56, generator=torch.Generator().manual_seed(B)).to(DEV)
    n = lib.keds_vit_workspace_bytes(C.byref(par), B)
    try:
        for lane in _lanes(flow):
            lib.keds_side_lane_enable(lane)
            plan = tc.plan_pass(flow, "vit", LAYERS, B, cls_only=bool(cls_only), split=_pass_split(lib, flow, 17, B, lane))
            chain = Chain(plan, blocks, front=_front(eng), inputs={"img": img})
            chain.run()
            assert chain.guards_intact() == []
            raw = chain.bufs["out"][:B]
            assert torch.isfinite(raw).all()
            for normalize in (0, 1):
                f32n = normalize and flow in ("f32", "x3")
                want = None if f32n else chain.out_norm if normalize else raw
                for fill in (0xFF, 0x00):
                    out = _out(B)
                    _in_sentinel(n, fill, lambda w_, nb: lib.keds_vit_run(C.byref(par), P(img), B, P(out), normalize, w_, nb, _lib.stream()), [out])
                    assert bool((out[B:] == rc.SENT).all())
                    if f32n:
                        _l2_held(out[:B], raw, f"vit {flow} B{B}")
                        continue
                    assert _same(out[:B], want), f"keds_vit_run {flow} B={B} cls_only={cls_only} normalize={normalize} lane={lane} fill={fill:#x}"
    finally:
        lib.keds_side_lane_enable(1)


@pytest.mark.parametrize("out_type", (0, 1, 2))
@pytest.mark.parametrize("B", (1, 16))
@pytest.mark.parametrize("flow", tc.FLOWS)
def test_vit_run_tokens_equals_its_chain(flow, B, out_type):
    """every tap and the tokens: the stream after each block, cast once (the fp16 stream of the folded flows, the fp32 stream else)"""
    lib = _lib.load()
    par, blocks, eng = _params(flow, "vit")
    img = torch.randn(B, 3, 56, 56, generator=torch.Generator().manual_seed(40 + B)).to(DEV)
    n = lib.keds_vit_workspace_bytes(C.byref(par), B)
    M = B * 17
    try:
        for lane in _lanes(flow):
            lib.keds_side_lane_enable(lane)
            plan = tc.plan_pass(flow, "vit_tokens", LAYERS, B, split=_pass_split(lib, flow, 17, B, lane))
            chain = Chain(plan, blocks, front=_front(eng), inputs={"img": img}, out_type=out_type)
            chain.run()
            assert chain.guards_intact() == [] and torch.isnan(chain.taps[LAYERS * M:].float()).all() and torch.isnan(chain.tokens[M:].float()).all()
            assert torch.isfinite(chain.taps[:LAYERS * M].float()).all()
            for fill in (0xFF, 0x00):
                out = _out(B)
                taps = torch.full((LAYERS * M + G, W), NAN, dtype=OUT_TYPE[out_type], device=DEV)
                toks = torch.full((M + G, W), NAN, dtype=OUT_TYPE[out_type], device=DEV)
                _in_sentinel(n, fill, lambda w_, nb: lib.keds_vit_run_tokens(C.byref(par), P(img), B, P(out), 0, P(taps), P(toks), out_type, w_, nb,
                                                                           _lib.stream()), [out, taps, toks])
                assert _same(taps, chain.taps) and _same(toks, chain.tokens), f"taps / tokens {flow} B={B} type {out_type} lane={lane} fill={fill:#x}"
                assert _same(out[:B], chain.bufs["out"][:B])
    finally:
        lib.keds_side_lane_enable(1)


def _text_inputs(B, splice, cols):
    g = torch.Generator().manual_seed(100 + B)
    tokens = torch.randint(0, VOCAB, (B, L), generator=g, dtype=torch.int32).to(DEV)
    img = torch.randn(B, splice[0], W, generator=g).to(DEV) if splice else None
    return {"tokens": tokens, "img_tokens": img, "rows": torch.tensor(cols, dtype=torch.int32, device=DEV)}


def _text_cases(B):
    """(read-out columns, seq_used, splice): columns spread over [0, 76] with 0 and 76 among them; seq_used 0, max + 1 and 77; one row
    declared outside the cut; spliced tokens at column 1 and ending at the read-out column"""
    spread = [[76], [0, 76, 33], [0, 76, 5, 20, 33, 61, 43]][(1, 3, 7).index(B)]
    short = [[20], [3, 20, 9], [3, 20, 9, 0, 14, 20, 17]][(1, 3, 7).index(B)]
    out = [(spread, 0, None), (spread, 77, (1, 1)), (short, 21, None), (short, 21, (3, 1)), (short, 21, (3, 18))]
    if B > 1:
        outside = list(short)
        outside[1] = 30                                  # declared outside the cut at 21: a NaN row
        out.append((outside, 21, None))
    return out


@pytest.mark.parametrize("trim", (0, 1, 2, 3))
@pytest.mark.parametrize("B", (1, 3, 7))
@pytest.mark.parametrize("flow", tc.FLOWS)
def test_text_run_equals_its_chain(flow, B, trim):
    lib = _lib.load()
    par, blocks, eng = _params(flow, "text")
    n = lib.keds_text_workspace_bytes(C.byref(par), B)
    try:
        _lib.check(lib.keds_text_trim_enable(trim), "keds_text_trim_enable")
        for cols, seq_used, splice in _text_cases(B):
            inp = _text_inputs(B, splice, cols)
            for lane in _lanes(flow):
                lib.keds_side_lane_enable(lane)
                Lx = seq_used if trim in (1, 2) and 0 < seq_used < L else L
                plan = tc.plan_pass(flow, "text", LAYERS, B, rows=cols, seq_used=seq_used, trim=trim, splice=splice,
                                    split=_pass_split(lib, flow, Lx, B, lane))
                assert plan.S == Lx
                chain = Chain(plan, blocks, front=_front(eng), inputs=inp)
                chain.run()
                assert chain.guards_intact() == []
                raw = chain.bufs["out"][:B]
                nan_rows = [not c < plan.S for c in cols]
                assert torch.isnan(raw).all(1).tolist() == nan_rows and torch.isfinite(raw[[not v for v in nan_rows]]).all()
                for normalize in (0, 1):
                    f32n = normalize and flow in ("f32", "x3")
                    want = None if f32n else chain.out_norm if normalize else raw
                    for fill in (0xFF, 0x00):
                        out = _out(B)
                        nt, c0 = splice if splice else (0, 0)
                        _in_sentinel(n, fill, lambda w_, nb: lib.keds_text_run_ex(C.byref(par), P(inp["tokens"]), P(inp["rows"]), P(inp["img_tokens"]), nt,
                                                                                c0, B, seq_used, P(out), normalize, w_, nb, _lib.stream()), [out])
                        assert bool((out[B:] == rc.SENT).all())
                        if f32n:
                            _l2_held(out[:B], raw, f"text {flow} B{B}")
                            continue
                        assert _same(out[:B], want), \
                            f"keds_text_run_ex {flow} B={B} trim={trim} seq_used={seq_used} splice={splice} cols={cols} normalize={normalize} lane={lane} fill={fill:#x}"
    finally:
        lib.keds_text_trim_enable(-1)
        lib.keds_side_lane_enable(1)


PACKED = {"256": ([1, 77, 5, 20, 33, 77, 43], 77), "257": ([1, 77, 5, 20, 33, 77, 44], 77), "max60": ([60, 1, 17, 60, 32], 60)}


@pytest.mark.parametrize("case", sorted(PACKED))
@pytest.mark.parametrize("flow", ("bf16", "unfolded", "fp16", "f32", "x3"))
def test_text_run_packed_equals_its_chain(flow, case):
    """packed rows: 256 rows exactly, 257 (255 zero rows run) and seq_max < L; the fp32 and split-fp16 attention on packed rows through
    keds_attention_f32_packed / keds_attention_x3_packed, entries onto the helpers the passes launch from"""
    lib = _lib.load()
    lens, seq_max = PACKED[case]
    B = len(lens)
    par, blocks, eng = _params(flow, "text")
    n = lib.keds_text_workspace_bytes(C.byref(par), B)
    off = [sum(lens[:b]) for b in range(B + 1)]
    rows = [off[b + 1] - 1 for b in range(B)]
    rows[1] = off[-1] + 2                                # outside [0, rows_total): a NaN row
    inp = _text_inputs(B, None, rows)
    inp["seq_off"] = torch.tensor(off, dtype=torch.int32, device=DEV)
    plan = tc.plan_pass(flow, "text_packed", LAYERS, B, lens=lens, seq_max=seq_max)
    chain = Chain(plan, blocks, front=_front(eng), inputs=inp)
    chain.run()
    assert chain.guards_intact() == []
    raw = chain.bufs["out"][:B]
    assert torch.isnan(raw).all(1).tolist() == [b == 1 for b in range(B)]
    stream = chain.bufs["h" if flow in ("bf16", "fp16") else "x"]
    assert torch.isfinite(stream[max(plan.valid, B):plan.M].float()).all(), "the zero rows must stay finite"
    for normalize in (0, 1):
        f32n = normalize and flow in ("f32", "x3")
        want = None if f32n else chain.out_norm if normalize else raw
        for fill in (0xFF, 0x00):
            out = _out(B)
            ws = _in_sentinel(n, fill, lambda w_, nb: lib.keds_text_run_packed(C.byref(par), P(inp["tokens"]), P(inp["seq_off"]), P(inp["rows"]), off[-1],
                                                                             seq_max, None, 0, 0, B, P(out), normalize, w_, nb, _lib.stream()), [out])
            if f32n:
                _l2_held(out[:B], raw, f"packed {flow} {case}")
            else:
                assert _same(out[:B], want), f"keds_text_run_packed {flow} {case} normalize={normalize} fill={fill:#x}"
            behind = ws[plan.M * W * 4:tc.pad256(B * seq_max) * W * 4]            # x rows behind rows_run keep the prefill
            assert behind.numel() > 0 and bool((behind == fill).all())


@pytest.mark.parametrize("out_type", (0, 1, 2))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("flow", tc.FLOWS)
def test_text_run_tokens_equals_its_chain(flow, B, out_type):
    lib = _lib.load()
    par, blocks, eng = _params(flow, "text")
    n = lib.keds_text_workspace_bytes(C.byref(par), B)
    inp = _text_inputs(B, None, [0] * B)
    try:
        for lane in _lanes(flow):
            lib.keds_side_lane_enable(lane)
            plan = tc.plan_pass(flow, "text_tokens", LAYERS, B, split=_pass_split(lib, flow, L, B, lane))
            chain = Chain(plan, blocks, front=_front(eng), inputs=inp, out_type=out_type)
            chain.run()
            assert chain.guards_intact() == []
            want = chain.bufs["tokens_out"][:B * L]
            assert torch.isfinite(want.float()).all()
            for fill in (0xFF, 0x00):
                out = torch.full((B * L + G, W), NAN, dtype=OUT_TYPE[out_type], device=DEV)
                _in_sentinel(n, fill, lambda w_, nb: lib.keds_text_run_tokens(C.byref(par), P(inp["tokens"]), B, P(out), out_type, w_, nb, _lib.stream()),
                             [out])
                assert torch.isnan(out[B * L:].float()).all() and _same(out[:B * L], want), f"keds_text_run_tokens {flow} B={B} type {out_type} lane={lane}"
    finally:
        lib.keds_side_lane_enable(1)


# ---- the comparison can fail: a chain with a defect differs from the pass ----------------------------------------------------------------
@pytest.mark.parametrize("name,flow,B,tail", [("rem_stats_row0", "fp8", 16, "all"), ("fc_stats_swapped", "bf16", 16, "all"),
                                              ("cls_ln_gamma", "fp16", 16, "cls"), ("rem_mlp_skipped", "fp8", 31, "all")])
def test_a_mutated_chain_differs_from_the_pass(name, flow, B, tail):
    lib = _lib.load()
    blocks = _blocks(flow, W, LAYERS)
    fp8, f32, f16 = FLAGS[flow]
    tp = _lib.TowerParams(W, LAYERS, HEADS, 17, 0, C.cast(blocks, C.POINTER(_lib.BlockParams)), fp8, int(tail == "cls"), f32, f16)
    M = B * 17
    x0 = torch.full((tc.pad256(M) + G, W), NAN, device=DEV)
    x0[:M] = torch.randn(M, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    plan = tc.plan(flow, "tower", LAYERS, B, S=17, tail=tail, width=W, heads=HEADS, causal=False)
    rows = torch.tensor(plan.out_rows, device=DEV)
    xt = _run_tower(tp, x0, B, 0xFF)
    clean, bad = Chain(plan, blocks, x0[:M]), Chain(tc.mutate(plan, name), blocks, x0[:M])
    clean.run()
    bad.run()
    assert torch.equal(xt[rows].view(torch.int32), clean.bufs["x"][rows].view(torch.int32))
    assert not _same(xt[rows], bad.bufs["x"][rows])


# ---- the chain is the arithmetic: every link within its kernel's bar, on the link's actual inputs ----------------------------------------
@pytest.mark.parametrize("tail", ("all", "cls"))
@pytest.mark.parametrize("B", (1, 15, 16, 31))
@pytest.mark.parametrize("flow", tc.FLOWS)
def test_every_link_within_its_kernels_bound(flow, B, tail):
    """the GEMM links through gemm_check.expected on Case / X3Case.from_operands (the statistics a RESID_STATS link adds through
    check_stats), the attention links through attention_check, the LayerNorm links through row_check.ln_reference: the existing checks
    with their existing constants; the MXFP8 links through mx_check.model_failures on MxCase.from_operands of the decoded bytes."""
    blocks = _blocks(flow, W, LAYERS)
    M = B * 17
    x = torch.randn(M, W, generator=torch.Generator().manual_seed(12 + B)).to(DEV)
    plan = tc.plan(flow, "tower", LAYERS, B, S=17, tail=tail, width=W, heads=HEADS, causal=False)
    chain = Chain(plan, blocks, x)
    chain.links, chain.eng = {}, _engine(flow)
    chain.run()
    assert chain.links
    for key, worst in sorted(chain.links.items()):
        report(f"tower_compositions.link.{key}.B{B}.{tail}", worst_ratio=worst)


@pytest.mark.parametrize("flow", tc.FLOWS)
def test_every_link_of_a_vit_and_a_text_pass_within_its_kernels_bound(flow):
    """the same on whole passes: the front ends and the read-out-row tail add im2col, cls_rows, embed_tokens (cut, splice, packed) and the
    gathers, held by bits, and the block links run on strided, gathered and packed rows"""
    B = 16
    par, blocks, eng = _params(flow, "vit")
    img = torch.randn(B, 3, 56, 56, generator=torch.Generator().manual_seed(2)).to(DEV)
    chains = [Chain(tc.plan_pass(flow, "vit", LAYERS, B), blocks, front=_front(eng), inputs={"img": img})]
    par_t, blocks_t, _ = _params(flow, "text")
    cols = [3, 20, 9, 0, 14, 20, 17]
    chains.append(Chain(tc.plan_pass(flow, "text", LAYERS, 7, rows=cols, seq_used=21, trim=1, splice=(3, 18)), blocks_t, front=_front(eng),
                        inputs=_text_inputs(7, (3, 18), cols)))
    chains.append(Chain(tc.plan_pass(flow, "text", LAYERS, 3, rows=[0, 76, 80], trim=0), blocks_t, front=_front(eng),
                        inputs=_text_inputs(3, None, [0, 76, 80])))                  # the read-out through its row map, one row outside
    chains.append(Chain(tc.plan_pass(flow, "text_tokens", LAYERS, 3), blocks_t, front=_front(eng), inputs=_text_inputs(3, None, [0] * 3)))
    if flow != "fp8":
        lens, seq_max = PACKED["257"]
        off = [sum(lens[:b]) for b in range(len(lens) + 1)]
        inp = _text_inputs(len(lens), None, [o - 1 for o in off[1:]])
        inp["seq_off"] = torch.tensor(off, dtype=torch.int32, device=DEV)
        chains.append(Chain(tc.plan_pass(flow, "text_packed", LAYERS, len(lens), lens=lens, seq_max=seq_max), blocks_t, front=_front(eng), inputs=inp))
    worst = {}
    for c in chains:
        c.links, c.eng = {}, eng
        c.run()
        for k, v in c.links.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert any(k.split(".", 1)[1].startswith("exact.") for k in worst)
    for key, v in sorted(worst.items()):
        report(f"tower_compositions.pass_link.{key}", worst_ratio=v)


@pytest.mark.parametrize("flow", ("bf16", "fp16"))
def test_vit_run_tokens_taps_of_the_side_lane_span(flow):
    """ViT-L geometry, 2 layers, B = 55: the 16-bit flows put 55 remainder rows on the side lane; every tap is taken per span on the lane
    that produced it, and equals the chain's stream after that block with the lane on and off"""
    lib = _lib.load()
    geo = dict(width=1024, layers=2, res=224)
    par, blocks, eng = _params(flow, "vit", **geo)
    B, S, w = 55, 257, 1024
    M = B * S
    img = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(55)).to(DEV)
    n = lib.keds_vit_workspace_bytes(C.byref(par), B)
    try:
        for lane in (1, 0):
            lib.keds_side_lane_enable(lane)
            assert lib.keds_tower_side_rows(w, S, B, 0) == (55 if lane else 0)
            plan = tc.plan_pass(flow, "vit_tokens", 2, B, width=w, heads=16, res=224, split=bool(lane))
            assert len(plan.spans) == (2 if lane else 1)
            chain = Chain(plan, blocks, front=_front(eng), inputs={"img": img}, out_type=1)
            chain.run()
            assert chain.guards_intact() == [] and torch.isfinite(chain.taps[:2 * M]).all()
            out = _out(B)
            taps = torch.full((2 * M + G, w), NAN, device=DEV)
            toks = torch.full((M + G, w), NAN, device=DEV)
            _in_sentinel(n, 0xFF, lambda w_, nb: lib.keds_vit_run_tokens(C.byref(par), P(img), B, P(out), 0, P(taps), P(toks), 1, w_, nb, _lib.stream()),
                         [out, taps, toks])
            assert _same(taps, chain.taps) and _same(toks, chain.tokens) and _same(out[:B], chain.bufs["out"][:B]), f"{flow} lane={lane}"
    finally:
        lib.keds_side_lane_enable(1)
