"""bf16-emulating statement of the fine pass: oracle/explicit.py plus the roundings of the bf16 route's kernels
(csrc/bf16_common.hip.h, bf16_sweeps.hip, bf16_color.hip, bf16_dw.hip).

TEST INFRASTRUCTURE ONLY (same rules as oracle/rnb_oracle.py).  RNB_VARIANT_BF16 keeps fp32 master weights, fp32
epilogues and fp32 accumulation; only what enters an MFMA or goes to HBM per point is rounded to bf16, round to nearest
even (the header comment of bf16_common.hip.h).  That arithmetic is deterministic up to summation order, so it can be
copied on the CPU: the sweeps of `FinePass` with `rb` applied at exactly the sites where the kernels round, and nowhere
else.

Rounding sites (`rb(x) = x.to(bfloat16).to(x.dtype)`; the name is the key of `Bf16FinePass.sites`).  "where" names the
kernel and the call that rounds: `pack2` and `to_bf` (bf16_common.hip.h) are the only two conversions, `k8_store_quad`
packs with `pack2`.  F, R, RA, FB = bf_forward_kernel, bf_reverse_kernel, bf_ra_kernel, bf_fb_kernel (bf16_sweeps.hip);
albedo fwd / bwd = bf_color_fwd_kernel / bf_color_bwd_kernel (bf16_color.hip).

  site    tensor                                  where                                     consumed by
  ------  --------------------------------------- ----------------------------------------  -----------------------------
  w       every MFMA weight matrix (W, W^T) of    bf_pack_kernel (pack2)                    F, R, RA, FB, feature head,
          the SDF hidden layers, the feature                                                albedo hidden layers (fwd,
          head and the albedo hidden layers                                                 bwd)
  pe      network input x and its PE columns      F: the encoding block (to_bf); the skip   F layer 0, skip layer, dW_0
                                                  layer's PE columns: epilogue, LDS store
  act     a_l = softplus(z_l)                     F epilogue: LDS store (to_bf) and the     F, sdf head, feature head, dW,
                                                  K8 save of g.a[l]                         sdf-head backward
  D       D_l = sigmoid(100 z_l)                  F epilogue: K8 save of g.D[l]             R, RA, FB
  gz      gz_l (R seed and sweep)                 R seed (pack2, to_bf); R epilogue: LDS    R, RA, dW
                                                  store and K8 save of g.gz[l - 1]
  feat    feature head output (bf16 albedo path)  F feature head: K8 store into cin8        albedo layer 0 (fwd, dW)
  cpe     pe(p), pe(n) columns of the albedo      albedo fwd: the encoding block (to_bf)    albedo layer 0 (fwd, dW)
          input
  cact    albedo hidden activations               albedo fwd epilogue: LDS store, K8 save   albedo fwd, output layer, dW,
                                                  of g.ac8[l]                               relu masks of the backward
  zc      albedo pre-activation adjoints          albedo bwd: the zc_{nc-1} block and the   albedo bwd products, dW, db
                                                  layer epilogue (LDS store, K8 save)
  fbar    feature adjoint                         albedo bwd: K8 store of g.fbar8 (bf16     FB head product, feature dW,
                                                  albedo path); FB: the load of g.fbar      feature db
                                                  (pack2; fp32 albedo path)
  geb     u_0 = J_pe nbar                         RA: the load of g.geb (to_bf), u_0 in K8  RA layer 0, skip layer, dW_0
  u       u_{l+1}                                 RA epilogue: LDS store, K8 save of        RA, dW, sdf-head backward
                                                  g.u[l + 1]
  zR      zR_l                                    RA epilogue: K8 save of g.zR[l]           FB
  zb      zb_l                                    FB epilogue: LDS store, K8 save of        FB, dW, db
                                                  g.zb[l]

Not rounded, as on the device: the sdf-head row and the albedo output layer (fp32 weights on bf16 activations: the "sdf
head" block of F, the "output layer + sigmoid" block of the albedo fwd), every epilogue (softplus, its derivative,
sigmoid, ReLU masks, the composite and its backward), g_e and the normal (the GE tile of R and its last block), the skip
connection's g_e share, the fp32 accumulators, every dW / db sum and the weight-norm backward.  The albedo network runs
in bf16 only where `bf16_color_supported` (bf16_color.hip) holds; otherwise it is the fp32 path (layers.hip), as on the
device.

Weights: `weights_from_packed` reads the device's own fp32 effective weights (the fp32 part of `packed`, after
rnb_weightnorm_fwd: the skip layer's 1/sqrt(2) folded in, the albedo layer-0 columns permuted to [feature | pe(p) |
pe(n)]).  A CPU weight norm could differ by one ulp, which can flip a weight's bf16 rounding: a systematic error
shared by every point, which no summation-order calibration covers.

Accumulation: every product and sum in `dtype` (float64: "emu64"; float32: "emu32").  `order="tiles"` sums the
weight and bias gradients over 64-point tiles in sequence (the device splits them over points), `order="mm"` leaves
them to one matrix product: two summation orders of the same rounded arithmetic.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import rnb_oracle as O
from .explicit import FinePass, pe_forward, pe_j, pe_jt, softplus100, weightnorm_backward

SITES = ("w", "pe", "act", "D", "gz", "feat", "cpe", "cact", "zc", "fbar", "geb", "u", "zR", "zb")
RS2 = 0.70710678118654752440


def rb(x: torch.Tensor) -> torch.Tensor:
    """Round to the nearest bf16 (ties to even), kept in x's dtype: v_cvt_pk_bf16_f32 / (__bf16) of the kernels.
    (float64 input goes through fp32 first, as the device rounds the fp32 result of its epilogue.)"""
    return x.to(torch.bfloat16).to(x.dtype)


def _pad32(x: int) -> int:
    return (x + 31) // 32 * 32


def packed_layout(mc: O.ModelConf) -> dict:
    """Float offsets of the packed weight buffer (csrc/layout.hip make_layout), SDF network and albedo network."""
    sc, cc = mc.sdf, mc.color
    nh, H = sc.n_layers, sc.d_hidden
    pe = 3 * (1 + 2 * sc.multires)
    Hp = _pad32(H)
    skip = sc.skip_in[0] if len(sc.skip_in) else -1
    off = 0
    hid = []
    for l in range(nh):
        K = pe if l == 0 else H
        N = H - pe if l + 1 == skip else H
        Kp = _pad32(K)
        e = dict(N=N, K=K, Np=Hp, Kp=Kp, w=off)
        off += Hp * Kp
        e["b"] = off
        off += Hp
        e["wT"] = off
        off += Kp * Hp
        hid.append(e)

    def place(N, K):
        nonlocal off
        e = dict(N=N, K=K, Np=_pad32(N), Kp=_pad32(K), w=off)
        off += e["Np"] * e["Kp"]
        e["b"] = off
        off += e["Np"]
        return e

    def transpose(e):
        nonlocal off
        e["wT"] = off
        off += e["Kp"] * e["Np"]

    F = sc.d_out - 1
    feat = place(F, H)
    transpose(feat)
    wsdf = off
    off += Hp
    bsdf = off
    off += 32
    pev = 3 * (1 + 2 * cc.multires_view)
    Cin = F + 2 * pev
    col = []
    for l in range(cc.n_layers):
        e = place(cc.d_hidden, Cin if l == 0 else cc.d_hidden)
        transpose(e)
        col.append(e)
    colo = place(cc.d_out, cc.d_hidden)
    return dict(hid=hid, feat=feat, wsdf=wsdf, bsdf=bsdf, col=col, colo=colo, F=F, pev=pev, Cin=Cin,
                Cinp=_pad32(Cin), total=_pad32(off))


def bf16_color_supported(mc: O.ModelConf) -> bool:
    """`bf16_color_supported` (csrc/bf16_color.hip) on the layout of `mc`."""
    L = packed_layout(mc)
    cc = mc.color
    if L["F"] != 256 or cc.d_hidden != 256:
        return False
    if L["Cinp"] > 320 or L["Cinp"] % 64 != 0 or L["Cinp"] - L["F"] > 64:
        return False
    return 1 <= cc.n_layers and 1 <= cc.d_out <= 4


def mirror_matrices(mc: O.ModelConf):
    """(name, float offset, N, K) of every matrix bf16_pack_weights mirrors (csrc/bf16_sweeps.hip), in its order."""
    L = packed_layout(mc)
    out = []
    for l, e in enumerate(L["hid"]):
        out += [(f"sdf.lin{l}", e["w"], e["Np"], e["Kp"]), (f"sdf.lin{l}^T", e["wT"], e["Kp"], e["Np"])]
    if L["F"] > 0:
        e = L["feat"]
        out += [("sdf.feat", e["w"], e["Np"], e["Kp"]), ("sdf.feat^T", e["wT"], e["Kp"], e["Np"])]
        for l, e in enumerate(L["col"]):
            out += [(f"color.lin{l}", e["w"], e["Np"], e["Kp"]), (f"color.lin{l}^T", e["wT"], e["Kp"], e["Np"])]
    return out


def unfragment(u16: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """bf16 bits of one mirrored matrix in MFMA-fragment order (the matrix loop of bf16_common.hip.h and
    `bf_pack_kernel`: fragment (nt, ks) = 64 units of 8 values,
    unit (h, c) = W[32 nt + c][16 ks + 8 h .. +8]) -> fp32 [N][K] row-major."""
    f = (u16.to(torch.int32) & 0xFFFF) << 16
    f = f.view(torch.float32).reshape(N // 32, K // 16, 2, 32, 8)     # nt, ks, h, c, j
    return f.permute(0, 3, 1, 2, 4).reshape(N, K)


def weights_from_packed(packed_f32: torch.Tensor, mc: O.ModelConf) -> dict:
    """The device's effective weights (CPU fp32 tensors) from the fp32 part of `packed`.  Hidden layer l: W [N_l, K_l]
    (the skip layer's 1/sqrt(2) folded in, its columns [a_{l-1} | pe]); the output layer as the sdf row `wsdf` and the
    feature head; the albedo layer 0 with its columns back in the reference order [pe(p) | pe(n) | feature]."""
    L = packed_layout(mc)
    P = packed_f32.detach().float().cpu()

    def mat(e, N=None, K=None):
        N, K = N or e["N"], K or e["K"]
        return P[e["w"]:e["w"] + e["Np"] * e["Kp"]].reshape(e["Np"], e["Kp"])[:N, :K].clone(), \
            P[e["b"]:e["b"] + N].clone()

    W, b = zip(*[mat(e) for e in L["hid"]])
    H = mc.sdf.d_hidden
    out = dict(W=list(W), b=list(b), wsdf=P[L["wsdf"]:L["wsdf"] + H].clone(), bsdf=P[L["bsdf"]:L["bsdf"] + 1].clone())
    F, pev = L["F"], L["pev"]
    if F > 0:
        out["Wf"], out["bf"] = mat(L["feat"])
        Wc, bc = [], []
        for l, e in enumerate(L["col"]):
            w, bb = mat(e)
            if l == 0:      # packed [feature | pe(p) | pe(n)] -> reference [pe(p) | pe(n) | feature]
                w = torch.cat([w[:, F:F + 2 * pev], w[:, :F]], 1)
            Wc.append(w)
            bc.append(bb)
        w, bb = mat(L["colo"])
        Wc.append(w)
        bc.append(bb)
        out["Wc"], out["bc"] = Wc, bc
    return out


def weights_from_params(p: O.Params, mc: O.ModelConf, dtype=torch.float64) -> dict:
    """The same dictionary computed from the parameters (weight norm in `dtype`, the skip factor folded in): for CPU
    tests that have no device."""
    from .explicit import eff_weights
    sc = mc.sdf
    n_lin = sc.n_layers + 1
    skip = sc.skip_in[0] if len(sc.skip_in) else -1
    q = {k: v.detach().to(dtype) for k, v in p.items()}
    W, b = eff_weights(q, "sdf", n_lin)
    W = [w * RS2 if l == skip else w for l, w in enumerate(W)]
    out = dict(W=W[:-1], b=b[:-1], wsdf=W[-1][0].clone(), bsdf=b[-1][:1].clone(), Wf=W[-1][1:].clone(),
               bf=b[-1][1:].clone())
    out["Wc"], out["bc"] = eff_weights(q, "color", mc.color.n_layers + 1)
    return out


class Bf16FinePass(FinePass):
    """`FinePass` with the bf16 variant's roundings.  `weights`: `weights_from_packed` (the device's) or
    `weights_from_params`; `sites`: the rounding sites that are on (default: all; an empty set is FinePass in `dtype`);
    `color_bf16`: the albedo network in bf16 (default: `bf16_color_supported`); `order`: "mm" or "tiles" (see the
    module docstring)."""

    def __init__(self, p: O.Params, mc: O.ModelConf, weights: dict, *, dtype=torch.float64, sites=SITES,
                 color_bf16: Optional[bool] = None, order: str = "mm"):
        q = {k: v.detach().to(dtype) for k, v in p.items()}
        super().__init__(q, mc)
        self.dt = dtype
        self.sites = set(sites)
        assert self.sites <= set(SITES), self.sites - set(SITES)
        self.color_bf16 = bf16_color_supported(mc) if color_bf16 is None else color_bf16
        assert order in ("mm", "tiles")
        self.order = order
        cv = lambda t: t.detach().to(dtype).cpu()
        rw = lambda t: self.r("w", cv(t))
        # self.W / self.b keep FinePass's meaning for the MFMA layers: bf16-rounded device weights
        self.W = [rw(w) for w in weights["W"]]
        self.b = [cv(v) for v in weights["b"]]
        self.wsdf, self.bsdf = cv(weights["wsdf"]), cv(weights["bsdf"])
        if "Wf" in weights:
            self.Wf, self.bfeat = rw(weights["Wf"]), cv(weights["bf"])
            nc = mc.color.n_layers
            # albedo hidden layers: bf16 MFMA weights on the bf16 path; the output layer is fp32 in both paths
            self.Wc = [(rw(w) if (self.color_bf16 and l < nc) else cv(w)) for l, w in enumerate(weights["Wc"])]
            self.bc = [cv(v) for v in weights["bc"]]

    # ------------------------------------------------------------------ helpers
    def r(self, site, x):
        return rb(x) if site in self.sites else x

    def _sum_rows(self, X, Y=None):
        """X^T Y (or the column sums of X) over points, in the configured order."""
        if self.order == "mm" or X.shape[0] <= 64:
            return X.sum(0) if Y is None else X.t() @ Y
        acc = None
        for i in range(0, X.shape[0], 64):
            t = X[i:i + 64].sum(0) if Y is None else X[i:i + 64].t() @ Y[i:i + 64]
            acc = t if acc is None else acc + t
        return acc

    # ------------------------------------------------------------------ F + R + C
    def forward_points(self, pts, use_color=True):
        sc, n_lin, skip = self.sc, self.n_lin, self.skip
        pts = pts.to(self.dt)
        x = pts * sc.scale
        e = self.r("pe", pe_forward(x, sc.multires) if sc.multires > 0 else x)
        self.x, self.e = x, e
        ins, acts, D = [], [], []
        h = e
        for l in range(n_lin - 1):
            if l == skip:
                h = torch.cat([h, e], 1)          # 1/sqrt(2) is folded into the device's W_skip
            ins.append(h)
            z = h @ self.W[l].t() + self.b[l]
            t = 100.0 * z
            # softplus_aD_fast; at 100 z > 20 a == z and D == 1 in fp32 (PyTorch's threshold in FinePass)
            D.append(self.r("D", torch.where(t > 20.0, torch.ones_like(z), torch.sigmoid(t))))
            h = self.r("act", softplus100(z))
            acts.append(h)
        ins.append(h)
        self.ins, self.acts, self.D = ins, acts, D
        sdf = (h @ self.wsdf[:, None] + self.bsdf) / sc.scale
        feat = h @ self.Wf.t() + self.bfeat if hasattr(self, "Wf") else h[:, :0]
        # R: the seed gz_{nh-1} = w_sdf * D_{nh-1} (fp32 w_sdf), then gz_{l-1} = (gz_l W_l) * D_{l-1}
        gz = [None] * (n_lin - 1)
        gz[n_lin - 2] = self.r("gz", self.wsdf[None, :] * D[n_lin - 2])
        g_e = torch.zeros_like(e)
        for l in range(n_lin - 2, 0, -1):
            g = gz[l] @ self.W[l]
            if l == skip:
                k = g.shape[1] - e.shape[1]
                g_e = g_e + g[:, k:]              # the skip connection's share: straight to g_e, fp32
                g = g[:, :k]
            gz[l - 1] = self.r("gz", g * D[l - 1])
        g_e = g_e + gz[0] @ self.W[0]
        self.gz = gz
        normal = pe_jt(x, g_e, sc.multires) if sc.multires > 0 else g_e
        self.sdf, self.normal, self.feat_fp32 = sdf, normal, feat    # (rnb_sdf_forward returns the fp32 feature)
        self.feat = self.r("feat", feat) if self.color_bf16 else feat
        if use_color:
            self.color_forward(pts, normal, self.feat)
        return sdf, self.feat, normal

    def color_forward(self, pts, normal, feat):
        cc = self.cc
        m = cc.multires_view
        assert cc.mode == "no_view_dir"
        cpe = torch.cat([pe_forward(pts, m), pe_forward(normal, m)], -1)
        if self.color_bf16:
            cpe = self.r("cpe", cpe)
        cin = torch.cat([cpe, feat], -1)
        self.cin = cin
        h = cin
        self.cacts = []
        nl = cc.n_layers + 1
        for l in range(nl):
            z = h @ self.Wc[l].t() + self.bc[l]
            if l < nl - 1:
                h = torch.relu(z)
                if self.color_bf16:
                    h = self.r("cact", h)
                self.cacts.append(h)
        self.albedo = torch.sigmoid(z) if cc.squeeze_out else z
        return self.albedo

    def forward(self, rays_o, rays_d, z_vals, lights_dir, **kw):
        cv = lambda t: None if t is None else t.to(self.dt)
        return super().forward(cv(rays_o), cv(rays_d), cv(z_vals), cv(lights_dir),
                               **{k: cv(v) if torch.is_tensor(v) else v for k, v in kw.items()})

    # ------------------------------------------------------------------ C' RA FB dW
    def _color_backward(self, albbar, grads):
        """C' of the bf16 albedo kernels (bf16_color.hip: bf_color_bwd_kernel, bf_color_out_bwd_kernel; the albedo dW
        jobs of bf16_dw_list in bf16_dw.hip): returns (fbar, the normal's share of the input adjoint)."""
        cc = self.cc
        nl = cc.n_layers + 1
        zo = albbar * self.albedo * (1 - self.albedo) if cc.squeeze_out else albbar
        # output layer (fp32 weights): dWo = zo^T a_last, dbo = colsum zo
        weightnorm_backward(self.p, "color", nl - 1, self._sum_rows(zo, self.cacts[-1]), self._sum_rows(zo), grads)
        zc = self.r("zc", (zo @ self.Wc[nl - 1]) * (self.cacts[-1] > 0).to(zo.dtype))
        for l in range(nl - 2, -1, -1):
            inp = self.cin if l == 0 else self.cacts[l - 1]
            weightnorm_backward(self.p, "color", l, self._sum_rows(zc, inp), self._sum_rows(zc), grads)
            inb = zc @ self.Wc[l]
            if l > 0:
                zc = self.r("zc", inb * (self.cacts[l - 1] > 0).to(inb.dtype))
        m = cc.multires_view
        pe_d = 3 * (1 + 2 * m) if m > 0 else 3
        fbar = self.r("fbar", inb[:, 2 * pe_d:])
        return fbar, inb[:, pe_d:2 * pe_d]

    def backward(self, gout: Dict[str, torch.Tensor]):
        gout = {k: v.to(self.dt) for k, v in gout.items()}
        sbar, nbar, albbar, dvar = self.composite_backward(gout)
        grads: Dict[str, torch.Tensor] = {"dev.variance": dvar}
        sc, cc, n_lin, skip = self.sc, self.cc, self.n_lin, self.skip
        with_color = not self.k["no_albedo"]
        fbar = None
        if with_color:
            if self.color_bf16:
                fbar, pen_bar = self._color_backward(albbar, grads)
            else:
                # fp32 albedo path (layers.hip): FinePass's C'; FB rounds the feature adjoint as it loads it (FB)
                zb = albbar * self.albedo * (1 - self.albedo) if cc.squeeze_out else albbar
                nl = cc.n_layers + 1
                for l in range(nl - 1, -1, -1):
                    inp = self.cin if l == 0 else self.cacts[l - 1]
                    weightnorm_backward(self.p, "color", l, self._sum_rows(zb, inp), self._sum_rows(zb), grads)
                    inb = zb @ self.Wc[l]
                    if l > 0:
                        zb = inb * (self.cacts[l - 1] > 0).to(inb.dtype)
                m = cc.multires_view
                pe_d = 3 * (1 + 2 * m) if m > 0 else 3
                fbar = self.r("fbar", inb[:, 2 * pe_d:])
                pen_bar = inb[:, pe_d:2 * pe_d]
            m = cc.multires_view
            nbar = nbar + (pe_jt(self.normal, pen_bar, m) if m > 0 else pen_bar)
        # RA (bf_ra_kernel): u_0 = geb; u_{l+1} = (u_l W_l^T) D_l, zR_l = 100 (u_l W_l^T - u_{l+1}) gz_l
        geb = self.r("geb", pe_j(self.x, nbar, sc.multires) if sc.multires > 0 else nbar)
        u = geb
        us, zR = [], []
        for l in range(n_lin - 1):
            if l == skip:
                u = torch.cat([u, geb], 1)
            us.append(u)
            v = u @ self.W[l].t()
            un = v * self.D[l]
            zR.append(self.r("zR", ((v - un) * self.gz[l]) * 100.0))
            u = self.r("u", un)
        # sdf-head row (bf_sdf_head_bwd_kernel): dw_sdf = sum (sbar / scale) a_last + u_last, db_sdf = sum sbar / scale
        sb = sbar * (1.0 / sc.scale)
        a_last = self.acts[-1]
        dW_out = [self._sum_rows(sb[:, None] * a_last + u)]
        db_out = [self._sum_rows(sb[:, None])]
        # FB (bf_fb_kernel): ab = fbar W_feat + (sbar / scale) w_sdf; zb_l = ab D_l + zR_l; ab = zb_l W_l
        ab = sb[:, None] * self.wsdf[None, :]
        if fbar is not None:
            ab = fbar @ self.Wf + ab
            dW_out.append(self._sum_rows(fbar, a_last))
            db_out.append(self._sum_rows(fbar))
        dW_out = torch.cat([dW_out[0][None, :]] + dW_out[1:], 0)
        db_out = torch.cat(db_out, 0)
        if fbar is None and self.mc.sdf.d_out > 1:
            dW_out = torch.cat([dW_out, torch.zeros(self.mc.sdf.d_out - 1, dW_out.shape[1], dtype=self.dt)], 0)
            db_out = torch.cat([db_out, torch.zeros(self.mc.sdf.d_out - 1, dtype=self.dt)], 0)
        weightnorm_backward(self.p, "sdf", n_lin - 1, dW_out, db_out, grads)
        zbs = [None] * (n_lin - 1)
        for l in range(n_lin - 2, -1, -1):
            zb = self.r("zb", ab[:, :self.W[l].shape[0]] * self.D[l] + zR[l])
            zbs[l] = zb
            # dW job of layer l (bf16_dw_list, bf16_dw.hip): gz_l^T u_l + zb_l^T in_l, bias from zb_l
            dW = self._sum_rows(self.gz[l], us[l]) + self._sum_rows(zb, self.ins[l])
            if l == skip:
                dW = dW * RS2           # the device's W_skip carries 1/sqrt(2); the parameter's gradient does not
            weightnorm_backward(self.p, "sdf", l, dW, self._sum_rows(zb), grads)
            if l > 0:
                ab = zb @ self.W[l]
        self.dbg = {"nbar": nbar, "fbar": fbar, "us": us, "zR": zR, "zb": zbs}
        return grads
