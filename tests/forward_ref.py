"""The forward counterpart of tests/backward_ref.py: the packed forward blob read back (mlp_layout.h), and fp64 references with worst-case
element-wise bounds for every layer of the fused forward kernels (nerf_amd/csrc/mlp_kernels.hip, mlp_core.h), one stage at a time.
Plain helper module (no fixtures): tests/test_gpu_forward_layers.py feeds it the blob ops.pack_weights wrote and the rows the training
forward dumped, tests/test_forward_ref_host.py feeds it an honest CPU emulation and seven planted faults.  The layout helpers
(feature_slot, enc_columns, slot_to_reference, ...) and the constants are backward_ref's.

THE BLOB.  `unpack` inverts the fragment stream from the description in mlp_layout.h: fragments layer by layer in consumption order
(feature-block pairs interleaved kg-major, an odd trailing block in plain kg order), element (lane, e) of fragment (fb, kg) = W[32 fb +
(lane & 31)][column(kg, lane >> 5, e)], stored [lane][e] in bf16 and [e >> 2][lane][e & 3] in fp32; the column is dmap_feature for hidden
inputs and pe_slot_column for encoded inputs; the bias table follows the stream, the fp32 fold (MipNeRF) the bias table.  The layout
tables are a parameter (LAYOUTS): the same code reads PropLayout, MipLayout, PropLayout128, MipLayout128 and RefLayout ('ref': 18
layers, the segment kind 'ide' = ide_slot_column for the 39 computed directional inputs, layer H = [bottle_neck ; the 11 head rows], the
(9, 19) IDE coefficient table behind the bias table; its stages and element-wise references live in tests/ref_forward_ref.py).  `pack` is
the same description written the other way round, fragment by fragment, for the host test.

THE LAYERS.  Every stage is compared AGAINST ITS OWN INPUTS: layer L from the dumped slot L - 1 (or the dumped encoding slot) and the
operands the blob holds.  With u = 2^-24, K = 16 NKG slots, s = in . W^T + b and A = |in| . |W|^T + |b| in fp64:

  hidden slot, bf16:   |got - relu(s)| <= 2^-8 |s| + 1.01 (K + 1) u A + (K + 1) 2^-126
  hidden slot, fp32:   |got - relu(s)| <= (K + 3) u A + (K + 1) 2^-126
      backward_ref.chain_tol's derivation with ONE more term: the bias enters the accumulation as the C operand of the block's first
      MFMA (mlp_core.h load_bias), so the chain adds K + 1 terms.  ReLU is 1-Lipschitz, so the bound on the pre-activation carries over
      to the activation and no element near zero needs or gets an exemption; where s < -tol the pre-activation the kernel holds is
      negative, so the dumped value must be exactly zero.  A truncating bf16 conversion (up to 2^-7 |s|) does not fit.
  sigma head, proposal density (fp32 outputs, both precisions; the kernels apply NO output transform: `sigma[t] = acc[0]`,
  `dens[t] = acc[0]`):   |got - s| <= (K + 3) u A + (K + 1) 2^-126      (bf16 operands make the products exact: fewer roundings, same bound)
  rgb = 1 / (1 + expf(-z)), z undumped, formed here from the dumped slot 7:   |got - sigmoid(z)| <= tol_z / 4 + 8 u,
      tol_z = (K + 3) u A + (K + 1) 2^-126.  Derivation of 8 (built with -ffp-contract=off and without fast-math, so the expression is
      three separately rounded operations): the kernel's fp32 z is within tol_z of z and |sigmoid'| <= 1/4: tol_z / 4.  t = expf(-z)
      carries a relative error of at most 3 ulp = 6 u (the OpenCL full-profile bound the device library documents for exp; HIP states
      1 ulp); d sigmoid / dt . t = -sigmoid (1 - sigmoid), magnitude <= 1/4: 1.5 u.  The addition 1 + t rounds once: relative u on a
      result <= 1: u.  The division: at most 2.5 ulp = 5 u relative (the same documents; hipcc's default is the correctly rounded one,
      0.5 u): 5 u.  Sum 7.5 u; 8 u pays for the second-order terms and for results flushed below 2^-126 (expf overflowing to +inf for
      z < -88 gives exactly 0 against sigmoid(z) < 2^-126).  Not fitted to what the kernel gives.
  mask records:  bit (m, f) of slot L == [dumped activation > 0], exactly.

THE FOLD (pack_kernels.hip fold_bottleneck_kernel).  Wf = a 256-term fused-multiply-add chain: within 257 u |W8a| |Wb| of the fp64
product (the bound of test_gpu_backward_layers._fold_matrix_ratio).  The folded bias is NOT the obvious analogue 257 u (|W8a| |bb| +
|b8|): the kernel runs the 256-term chain over W8a bb from zero and then adds b8 in one separately rounded addition,
`bf = s + b8`, so  |bf - (W8a bb + b8)| <= ((1 + u)^256 - 1) |W8a| |bb| + u |s^ + b8| <= 258 u |W8a| |bb| + u |b8|
-- one u more on the product term (the final addition rounds the whole sum), 257 times less on |b8| (it is rounded once).

None of these is fitted to what the kernels produce."""
import torch

import backward_ref as R

U24, TINY, BF16_HALF_ULP = R.U24, R.TINY, R.BF16_HALF_ULP
TILE = {"bf16": 256, "fp32": 128}            # samples per forward tile of the training kernels (and of the bf16 render kernels)
SIGMOID_C = 8.0


# ------------------------------------------------------------------------------------------------ layout tables (mlp_layout.h)
class Layout:
    """One network's stream: per layer NKG / NFB / START / BIAS_OFF as in the header, the real output rows, the width of the reference
    matrix, its K segments (kind 'pe' | 'd', K groups, first reference column, PE levels, valid width) and the master tensor it packs
    (an index into the state_dict order, or 'fold' = [Wf | rgb_layer.0[:, 256:]] with the folded bias)."""

    def __init__(self, name, nkg, nfb, start, bias_off, n_frags, n_bias, rows, in_f, src, segs, used_frags=None, fold=False, n_ide=0):
        self.name, self.NKG, self.NFB, self.START, self.BIAS_OFF = name, nkg, nfb, start, bias_off
        self.N_FRAGS, self.N_BIAS, self.rows, self.in_f, self.src, self.fold = n_frags, n_bias, rows, in_f, src, fold
        self.N_IDE = n_ide                                                  # floats of the IDE coefficient table behind the bias table (RefLayout)
        self.USED_FRAGS = n_frags if used_frags is None else used_frags
        self.N_LAYERS = len(nkg)
        self.segs = [segs.get(l, [("d", nkg[l], 0, 0, in_f[l])]) for l in range(self.N_LAYERS)]

    def stream_bytes(self, prec):
        return self.N_FRAGS * (1024 if prec == "bf16" else 2048)

    def packed_bytes(self, prec):
        return self.stream_bytes(prec) + 4 * (self.N_BIAS + self.N_IDE) + ((128 * 256 + 128) * 4 if self.fold else 0)


_PE10 = ("pe", 4, 0, 10, 63)
_DIR_IN = [("d", 8, 0, 0, 128), ("ide", 3, 128, 0, 39)]            # [bottle_neck 128 | IDE real 19 | IDE imag 19 | n.d]
IDE_ROWS, IDE_TERMS = 9, 19                                       # the (9, 19) coefficient table; RefLayout pads it to N_IDE = 176 floats
LAYOUTS = {
    "prop": Layout("prop", (4, 16, 16, 16, 16), (8, 8, 8, 8, 1), (0, 32, 160, 288, 416), (0, 256, 512, 768, 1024), 432, 1056,
                   (256, 256, 256, 256, 1), (63, 256, 256, 256, 256), (0, 1, 2, 3, 4), {0: [_PE10]}),
    "prop128": Layout("prop128", (4, 8, 8, 8, 8), (4, 4, 4, 4, 1), (0, 16, 48, 80, 112), (0, 128, 256, 384, 512), 128, 544,
                      (128, 128, 128, 128, 1), (63, 128, 128, 128, 128), (0, 1, 2, 3, 4), {0: [_PE10]}, used_frags=120),
    #                l1.0 l1.2 l1.4 l1.6 l2.0 l2.2 l2.4 sigma rgb0' rgb2
    "mip": Layout("mip", (4, 16, 16, 16, 20, 16, 16, 16, 18, 8), (8, 8, 8, 8, 8, 8, 8, 1, 4, 1),
                  (0, 32, 160, 288, 416, 576, 704, 832, 848, 920), (0, 256, 512, 768, 1024, 1280, 1536, 1792, 1824, 1952), 928, 1984,
                  (256, 256, 256, 256, 256, 256, 256, 1, 128, 3), (63, 256, 256, 256, 319, 256, 256, 256, 283, 128),
                  (0, 1, 2, 3, 4, 5, 6, 8, "fold", 10),
                  {0: [_PE10], 4: [_PE10, ("d", 16, 63, 0, 256)], 8: [("d", 16, 0, 0, 256), ("pe", 2, 256, 4, 27)]}, fold=True),
    "mip128": Layout("mip128", (4, 8, 8, 8, 12, 8, 8, 16, 18, 8), (4, 4, 4, 4, 4, 4, 8, 1, 4, 1),
                     (0, 16, 48, 80, 112, 160, 192, 256, 272, 344), (0, 128, 256, 384, 512, 640, 768, 1024, 1056, 1184), 352, 1216,
                     (128, 128, 128, 128, 128, 128, 256, 1, 128, 3), (63, 128, 128, 128, 191, 128, 128, 256, 283, 128),
                     (0, 1, 2, 3, 4, 5, 6, 8, "fold", 10),
                     {0: [_PE10], 4: [_PE10, ("d", 8, 63, 0, 128)], 8: [("d", 16, 0, 0, 256), ("pe", 2, 256, 4, 27)]}, fold=True),
    # RefLayout:      S0  S1  S2  S3  S4  S5  S6  S7  H   D0  D1  D2  D3  D4  D5  D6  D7  R
    # src = index into the 20 tensors pack_ref takes (spatial 0..7, bottle_neck 8, heads (11, 256) 9, directional 10..17, spec head 18,
    # IDE table 19); 'H' = [bottle_neck 128 rows ; the 11 head rows: normal 0-2, roughness 3, diffuse 4-6, density 7, tint 8-10]
    "ref": Layout("ref", (4, 16, 16, 16, 20, 16, 16, 16, 16, 11, 16, 16, 16, 27, 16, 16, 16, 16), (8, 8, 8, 8, 8, 8, 8, 8, 5, 8, 8, 8, 8, 8, 8, 8, 8, 1),
                  (0, 32, 160, 288, 416, 576, 704, 832, 960, 1040, 1128, 1256, 1384, 1512, 1728, 1856, 1984, 2112),
                  (0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2208, 2464, 2720, 2976, 3232, 3488, 3744, 4000, 4256), 2128, 4288,
                  (256,) * 8 + (139,) + (256,) * 8 + (3,), (63, 256, 256, 256, 319, 256, 256, 256, 256, 167, 256, 256, 256, 423, 256, 256, 256, 256),
                  (0, 1, 2, 3, 4, 5, 6, 7, "H", 10, 11, 12, 13, 14, 15, 16, 17, 18),
                  {0: [_PE10], 4: [_PE10, ("d", 16, 63, 0, 256)], 9: _DIR_IN, 13: _DIR_IN + [("d", 16, 167, 0, 256)]}, n_ide=176),
}


def consumption_order(nfb, nkg):
    """(feature block, K group) of every fragment of a layer, in stream order"""
    order = []
    for g in range(nfb // 2):
        for kg in range(nkg):
            order += [(2 * g, kg), (2 * g + 1, kg)]
    if nfb % 2:
        order += [(nfb - 1, kg) for kg in range(nkg)]
    return order


def ide_slot_column(q, h):
    """column (relative to the 39 computed directional inputs [real 19 | imag 19 | n.d]) that IDE slot (q, h) holds, or -1 (mlp_layout.h)"""
    if q < IDE_TERMS:
        return (IDE_TERMS if h else 0) + q
    return 38 if (q == IDE_TERMS and not h) else -1


def slot_column(segs, kg, h, e):
    """reference column of K slot (kg, h, e) of a layer, or -1 for zero padding"""
    for kind, n, col0, L, width in segs:
        if kg < n:
            c = R.pe_slot_column(8 * kg + e, h, L) if kind == "pe" else (ide_slot_column(8 * kg + e, h) if kind == "ide" else R.dmap_feature(kg, h, e))
            return col0 + c if 0 <= c < width else -1
        kg -= n
    raise IndexError("K group beyond the layer's segments")


_MAPS = {}


def index_map(lay, l, prec):
    """-> (pos, row, col): for every element of layer l's fragments its position in the stream (in elements), the output row and the
    reference column it holds; col = -1 or row >= rows[l]: a padding element"""
    key = (lay.name, l, prec)
    if key not in _MAPS:
        nkg, nfb = lay.NKG[l], lay.NFB[l]
        order = torch.tensor(consumption_order(nfb, nkg))                                            # (F, 2)
        cols = torch.tensor([[[slot_column(lay.segs[l], kg, h, e) for e in range(8)] for h in range(2)] for kg in range(nkg)])
        F = order.shape[0]
        lane, e = torch.arange(64).view(1, 64, 1), torch.arange(8).view(1, 1, 8)
        frag = (lay.START[l] + torch.arange(F)).view(F, 1, 1)
        inner = lane * 8 + e if prec == "bf16" else (e >> 2) * 256 + lane * 4 + (e & 3)
        pos = (frag * 512 + inner).expand(F, 64, 8)
        row = (32 * order[:, 0].view(F, 1, 1) + (lane & 31)).expand(F, 64, 8)
        col = cols[order[:, 1]][:, lane.view(64) >> 5, :]                                             # (F, 64, 8)
        _MAPS[key] = (pos.reshape(-1).contiguous(), row.reshape(-1).contiguous(), col.reshape(-1).contiguous())
    return _MAPS[key]


def map_is_bijection(lay, prec):
    """the index maps of all layers tile [0, USED_FRAGS * 512) exactly once, and every layer's real elements hit every entry of its
    (rows, in_f) matrix exactly once"""
    seen = torch.zeros(lay.N_FRAGS * 512, dtype=torch.int64)
    for l in range(lay.N_LAYERS):
        pos, row, col = index_map(lay, l, prec)
        seen.index_add_(0, pos, torch.ones_like(pos))
        real = (row < lay.rows[l]) & (col >= 0)
        hit = torch.zeros(lay.rows[l] * lay.in_f[l], dtype=torch.int64)
        hit.index_add_(0, row[real] * lay.in_f[l] + col[real], torch.ones(int(real.sum()), dtype=torch.int64))
        if not bool((hit == 1).all()) or int(col.max()) >= lay.in_f[l]:
            return False
    return bool((seen[: lay.USED_FRAGS * 512] == 1).all()) and not bool(seen[lay.USED_FRAGS * 512:].any())


class Unpacked:
    """w[l] (rows, in_f) / pad[l] in the stream's element type, b[l] (rows,) / bpad[l] fp32, tail = the stream's padding fragments,
    fold_w (128, 256) / fold_b (128,) = the fp32 fold behind the bias table (MipNeRF layouts), ide (9, 19) = the IDE coefficient table
    behind the bias table (RefLayout; its 5 padding floats are neither written by the pack nor read by the kernel, and are not returned)"""


def unpack(blob, lay, prec):
    assert blob.dtype == torch.uint8 and blob.numel() == lay.packed_bytes(prec), (blob.numel(), lay.packed_bytes(prec))
    sb = lay.stream_bytes(prec)
    stream = blob[:sb].view(torch.bfloat16 if prec == "bf16" else torch.float32)
    bias = blob[sb: sb + 4 * lay.N_BIAS].view(torch.float32)
    u = Unpacked()
    u.w, u.pad, u.b, u.bpad = [], [], [], []
    for l in range(lay.N_LAYERS):
        pos, row, col = (t.to(blob.device) for t in index_map(lay, l, prec))
        vals = stream[pos]
        real = (row < lay.rows[l]) & (col >= 0)
        w = torch.zeros((lay.rows[l], lay.in_f[l]), dtype=stream.dtype, device=blob.device)
        w[row[real], col[real]] = vals[real]
        u.w.append(w)
        u.pad.append(vals[~real])
        tab = bias[lay.BIAS_OFF[l]: lay.BIAS_OFF[l] + 32 * lay.NFB[l]]
        u.b.append(tab[: lay.rows[l]].clone())
        u.bpad.append(tab[lay.rows[l]:].clone())
    u.tail = stream[lay.USED_FRAGS * 512:].clone()
    if lay.fold:
        f = blob[sb + 4 * lay.N_BIAS:].view(torch.float32)
        u.fold_w, u.fold_b = f[: 128 * 256].view(128, 256).clone(), f[128 * 256:].clone()
    if lay.N_IDE:
        u.ide = blob[sb + 4 * lay.N_BIAS:].view(torch.float32)[: IDE_ROWS * IDE_TERMS].view(IDE_ROWS, IDE_TERMS).clone()
    return u


def layer_masters(lay, ws, bs, fold_w=None, fold_b=None):
    """the (rows, in_f) fp32 matrix and bias every layer packs, from the master tensors in state_dict order"""
    mats, biases = [], []
    for l, src in enumerate(lay.src):
        if src == "fold":
            mats.append(torch.cat((fold_w.float(), ws[9].detach().float()[:, 256:]), dim=1))
            biases.append(fold_b.float())
        elif src == "H":
            mats.append(torch.cat((ws[8].detach().float(), ws[9].detach().float()), dim=0))
            biases.append(torch.cat((bs[8].detach().float(), bs[9].detach().float()), dim=0))
        else:
            mats.append(ws[src].detach().float())
            biases.append(bs[src].detach().float())
    return mats, biases


def pack(lay, prec, mats, biases, fold_w=None, fold_b=None, ide=None):
    """the Python packer of the host test: mlp_layout.h written forwards, one fragment at a time -> uint8 blob"""
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    stream = torch.full((lay.N_FRAGS * 512,), float("nan")).to(dt)
    bias = torch.full((lay.N_BIAS,), float("nan"))
    for l in range(lay.N_LAYERS):
        padded = torch.zeros((32 * lay.NFB[l], lay.in_f[l] + 1))                                     # last column: what a padding slot reads
        padded[: lay.rows[l], : lay.in_f[l]] = mats[l]
        f = lay.START[l]
        for fb, kg in consumption_order(lay.NFB[l], lay.NKG[l]):
            block = torch.empty((64, 8))
            for h in range(2):
                for e in range(8):
                    c = slot_column(lay.segs[l], kg, h, e)
                    block[32 * h: 32 * h + 32, e] = padded[32 * fb: 32 * fb + 32, c]                 # (c = -1: the zero column)
            block = block.to(dt)
            flat = block.reshape(-1) if prec == "bf16" else block.view(64, 2, 4).permute(1, 0, 2).reshape(-1)
            stream[f * 512: (f + 1) * 512] = flat
            f += 1
        bias[lay.BIAS_OFF[l]: lay.BIAS_OFF[l] + 32 * lay.NFB[l]] = 0.0
        bias[lay.BIAS_OFF[l]: lay.BIAS_OFF[l] + lay.rows[l]] = biases[l]
    stream[lay.USED_FRAGS * 512:] = 0
    parts = [stream.view(torch.uint8), bias.view(torch.uint8)]
    if lay.fold:
        parts += [fold_w.float().contiguous().view(-1).view(torch.uint8), fold_b.float().contiguous().view(torch.uint8)]
    if lay.N_IDE:
        tab = torch.zeros(lay.N_IDE)
        tab[: IDE_ROWS * IDE_TERMS] = ide.float().reshape(-1)
        parts.append(tab.view(torch.uint8))
    return torch.cat(parts)


def fold_bounds(w8, b8, wb, bb):
    """fp64 (Wf, tol_Wf, bf, tol_bf) of the pack-time fold (module docstring: THE FOLD)"""
    w8a, wb, bb, b8 = w8.double()[:, :256], wb.double(), bb.double(), b8.double()
    return (w8a @ wb, 257 * U24 * (w8a.abs() @ wb.abs()), w8a @ bb + b8, 258 * U24 * (w8a.abs() @ bb.abs()) + U24 * b8.abs())


# ------------------------------------------------------------------------------------------------ the dump
WIDTH = {"prop": (256, 256, 256, 256), "mip": (256, 256, 256, 256, 256, 256, 256, 128)}
ENC_SLOT = {"prop": 4, "mip": 8}
ENC_WIDTH = {"prop": 64, "mip": 96}
DUMP_SLOTS = {"prop": 5, "mip": 9, "ref": 17}                     # PROP_DUMP_SLOTS, MIP_DUMP_SLOTS, REF_DUMP_SLOTS (mlp_layout.h)


def geometry(prec, M):
    """-> (subtiles, layer stride in bytes) of a training dump"""
    tile = TILE[prec]
    n_sub = (M + tile - 1) // tile * (tile // 32)
    return n_sub, n_sub * 16 * (1024 if prec == "bf16" else 2048)


_MASK_TABLE = {}


def mask_rows(block, n_features):
    """one slot's ReLU bit-mask records (uint8, 1 KiB per subtile) -> bool (32 n_sub, n_features) through backward_ref.mask_bit"""
    if n_features not in _MASK_TABLE:
        tab = [[R.mask_bit(j, f) for f in range(n_features)] for j in range(32)]
        _MASK_TABLE[n_features] = (torch.tensor([[t[0] for t in r] for r in tab]), torch.tensor([[t[1] for t in r] for r in tab]))
    byte, bit = (t.to(block.device) for t in _MASK_TABLE[n_features])
    rec = block.view(-1, 1024).to(torch.int32)
    return ((rec[:, byte] >> bit) & 1).bool().reshape(-1, n_features)


def mask_block(dump, net, prec, M, slot):
    n_sub, ls = geometry(prec, M)
    slots = DUMP_SLOTS[net]
    assert dump.numel() == slots * (ls + n_sub * 1024)
    return dump[slots * ls + slot * n_sub * 1024: slots * ls + (slot + 1) * n_sub * 1024]


# ------------------------------------------------------------------------------------------------ the stages
# (name, stream layer, kind, inputs: dump slots / 'enc' / 'dir' concatenated in the reference's column order, output: dump slot or columns of `out`)
STAGES = {
    "prop": [("h0", 0, "hidden", ("enc",), 0), ("h1", 1, "hidden", (0,), 1), ("h2", 2, "hidden", (1,), 2), ("h3", 3, "hidden", (2,), 3),
             ("density", 4, "linear", (3,), slice(0, 1))],
    "mip": [("h0", 0, "hidden", ("enc",), 0), ("h1", 1, "hidden", (0,), 1), ("h2", 2, "hidden", (1,), 2), ("h3", 3, "hidden", (2,), 3),
            ("h4", 4, "hidden", ("enc", 3), 4), ("h5", 5, "hidden", (4,), 5), ("h6", 6, "hidden", (5,), 6),
            ("sigma", 7, "linear", (6,), slice(3, 4)), ("h7", 8, "hidden", (6, "dir"), 7), ("rgb", 9, "sigmoid", (7,), slice(0, 3))],
}


def hidden_tol(s, a, K, prec):
    if prec == "bf16":
        return BF16_HALF_ULP * s.abs() + 1.01 * (K + 1) * U24 * a + (K + 1) * TINY
    return (K + 3) * U24 * a + (K + 1) * TINY


def linear_tol(a, K):
    return (K + 3) * U24 * a + (K + 1) * TINY


def noisy_tol(s, a, add, K, prec):
    """round(s + add) without ReLU (Ref-NeRF's bottle-neck): the linear bound t on s, one fp32 addition of the computed s^ and add
    (|s^ + add| <= |s| + t + |add|), and in bf16 the half-ulp conversion of the computed sum (|sum^| <= |s + add| + t1)"""
    t = linear_tol(a, K)
    t1 = t + U24 * (s.abs() + t + add.abs())
    return t1 + BF16_HALF_ULP * ((s + add).abs() + t1) if prec == "bf16" else t1


def check_stage(got, x, w, b, K, prec, kind, chunk=1 << 15, add=None):
    """One stage against its own inputs: got (M, N), x (M, in_f) the dumped input rows, w (N, in_f) / b (N,) the blob's operands.
    -> dict: worst = max(err / tol) over EVERY element, where = (sample, feature) of it, neg_nonzero = hidden elements with s < -tol
    that are not exactly zero.  kind 'noisy': got = round(s + add), add (M, N) or None = zero."""
    N = got.shape[1]
    w64, b64 = w.double(), b.double()
    wa, ba = w64.abs(), b64.abs()
    worst, where, neg_nonzero = 0.0, (0, 0), 0
    for i in range(0, got.shape[0], chunk):
        xx = x[i: i + chunk].double()
        s, a = xx @ w64.t() + b64, xx.abs() @ wa.t() + ba
        g = got[i: i + chunk].double()
        if kind == "hidden":
            tol, want = hidden_tol(s, a, K, prec), torch.relu(s)
            neg_nonzero += int(((s < -tol) & (g != 0)).sum())
        elif kind == "linear":
            tol, want = linear_tol(a, K), s
        elif kind == "noisy":
            ad = torch.zeros_like(s) if add is None else add[i: i + chunk].double()
            tol, want = noisy_tol(s, a, ad, K, prec), s + ad
        else:
            tol, want = linear_tol(a, K) / 4 + SIGMOID_C * U24, torch.sigmoid(s)
        ratio = (g - want).abs() / tol
        ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
        r = float(ratio.max())
        if r > worst:
            k = int(ratio.argmax())
            worst, where = r, (i + k // N, k % N)
    return {"worst": worst, "where": where, "neg_nonzero": neg_nonzero}


def encodings(net, enc):
    """encoding slot rows -> the reference's column order ((M, 63), (M, 27) or None); the padding features must be exactly zero"""
    ex, pad = R.slot_to_reference(enc[:, :64], 10)
    assert not bool((pad != 0).any()), "a padding feature of the position encoding slot is not zero"
    if net == "prop":
        return ex, None
    ed, pad = R.slot_to_reference(enc[:, 64:96], 4)
    assert not bool((pad != 0).any()), "a padding feature of the direction encoding slot is not zero"
    return ex, ed


def check_forward(net, prec, lay, u, acts, enc, out, masks=None):
    """Every stage of one forward run.  acts[L] = rows of dump slot L, enc = rows of the encoding slot, out = the kernel's output
    ((M,) density or (M, 4) rgbo), u = the unpacked blob, masks[L] = bool rows of slot L's mask records (optional).
    -> {stage: check_stage report}, plus 'mask' -> {'worst': number of mask bits that differ from [act > 0], 'where': the first}"""
    ex, ed = encodings(net, enc)
    out = out.reshape(out.shape[0], -1)
    rep = {}
    for name, l, kind, ins, dst in STAGES[net]:
        x = torch.cat([ex if i == "enc" else (ed if i == "dir" else acts[i]) for i in ins], dim=1)
        got = acts[dst] if kind == "hidden" else out[:, dst]
        rep[name] = check_stage(got, x, u.w[l], u.b[l], 16 * lay.NKG[l], prec, kind)
    if masks is not None:
        bad, first = 0, None
        for L, m in masks.items():
            diff = m != (acts[L] > 0)
            n = int(diff.sum())
            if n and first is None:
                k = int(diff.reshape(-1).float().argmax())
                first = (L, k // diff.shape[1], k % diff.shape[1])
            bad += n
        rep["mask"] = {"worst": float(bad), "where": first, "neg_nonzero": 0}
    return rep


def ratios(rep):
    """{stage: the figure its gate takes}: max(err / tol), or inf where an element that had to be exactly zero is not; 'mask': the
    number of wrong mask bits (limit 0)"""
    return {k: (float("inf") if v["neg_nonzero"] else v["worst"]) for k, v in rep.items()}


def assert_forward(what, rep):
    bad = {k: v for k, v in rep.items() if v["neg_nonzero"] or not v["worst"] <= (0.0 if k == "mask" else 1.0)}
    assert not bad, "%s: beyond the bound in %s" % (what, ", ".join(
        "%s (%.3g at %s, %d not zero where s < -tol)" % (k, v["worst"], v["where"], v["neg_nonzero"]) for k, v in sorted(bad.items())))
