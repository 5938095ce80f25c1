"""The sweep behind tests/golden/attn_plan.json: which attention kernel every descriptor gets.

One place for the cells, shared by tools/record_attn_plan.py (records what the library answers, on an MI355X),
tests/test_attn_plan.py (the plan of csrc/attn_plan.h must answer the same, on the CPU) and tests/test_gpu_attn_plan.py (the
built library must still answer the same). A cell is a dict of the fields that differ from DEFAULTS / ROWS_DEFAULTS;
`query(cell)` derives every number of the descriptor from it (no torch), `Buffers(cell, dev)` allocates zero-filled, guarded
buffers of exactly that size and fills the descriptor.

Every cell is either a valid descriptor of its size or one that the launcher rejects before it launches anything, under
every switch setting of SWITCHED: misaligned and wrong leading dimensions appear only in shapes whose checks come before
the first routing decision."""
from __future__ import annotations

GUARD_ROWS = 5
VIT_ENDS = {193: 41, 256: 42, 257: 51, 320: 52, 321: 61, 384: 62, 385: 71, 448: 72}      # tests/test_gpu_attn_conformance.py
# the plan switches, each flipped alone (index 0: the shipped defaults)
SWITCHED = [{}, {"attn_vit": 0}, {"attn_vit": 1}, {"attn_vit_len": 0}, {"attn_decode": 0}, {"attn_prefill_dma": 0},
            {"attn_nq": 1}, {"attn_nq": 2}, {"attn_combine32": 0}, {"attn_light_first": 1}]

DEFAULTS = dict(kind="attn", dtype="bf16", hd=128, q_len=1, q_pos0=0, causal=0, pre=0, hq=4, hkv=4, nsplit=1, cu=None, row_lo=0,
                force_rowwise=0, ws="exact", head_major=0, ldv_pad=0, ld_off=None, head_stride=None, hint=0)
ROWS_DEFAULTS = dict(kind="rows", rows=3, hq=8, hkv=2, hd=128, prefix_len=100, tail_len=3, tail_max=8, nsplit=2, slot=0,
                     slot_ld="ok", ws="exact")
HEADS = [(4, 4), (7, 1), (34, 2)]      # the last: 17 query heads per kv head, no GQA packing


def cells():
    """the base cells in the order they run; every one runs under each setting of SWITCHED"""
    out = []

    def add(**kw):
        out.append(kw)

    # ---- general / prompt / decode
    for hd in (64, 72, 128, 256):
        for dtype in ("bf16", "fp32"):
            for q_len in (1, 2, 127, 129):
                for q_pos0 in (0, 70):
                    add(hd=hd, dtype=dtype, q_len=q_len, q_pos0=q_pos0, causal=1)
    for hd in (72, 128):
        for q_len in (1, 2, 127, 129):
            for causal, q_pos0 in ((0, 0), (1, 0), (1, 70)):
                for pre in (0, 1):
                    for hq, hkv in HEADS:
                        add(hd=hd, q_len=q_len, q_pos0=q_pos0, causal=causal, pre=pre, hq=hq, hkv=hkv)
    for hd in (72, 128):
        for q_len in (1, 2):
            for pre in (0, 1):
                for hq, hkv in HEADS:
                    for nsplit in (2, 128, 129):
                        add(hd=hd, q_len=q_len, q_pos0=70, causal=1, pre=pre, hq=hq, hkv=hkv, nsplit=nsplit)
    for hd in (72, 128):
        for ws in ("short", "absent"):
            add(hd=hd, q_pos0=70, causal=1, pre=1, hq=7, hkv=1, nsplit=2, ws=ws)
    add(hd=64, q_pos0=70, causal=1, nsplit=2, ws="absent")                      # the row-wise kernel does not split
    add(hd=128, dtype="fp32", q_pos0=70, causal=1, nsplit=2, ws="absent")
    for hd in (72, 128):
        for causal in (0, 1):
            for pre in (0, 1):
                for hq, hkv in HEADS[:2]:
                    add(hd=hd, cu=[0, 60, 189], causal=causal, pre=pre, hq=hq, hkv=hkv)
        add(hd=hd, cu=[0, 60, 189], causal=1, pre=1, nsplit=2)
    add(hd=64, dtype="fp32", cu=[0, 60, 189])
    for hd in (72, 128):
        for pre in (0, 1):
            for q_len in (2, 129):
                add(hd=hd, q_len=q_len, pre=pre, row_lo=1)
        add(hd=hd, q_len=2, row_lo=1, nsplit=2)
        for pre in (0, 1):
            add(hd=hd, q_len=2, pre=pre, force_rowwise=1)
    add(hd=64, dtype="fp32", q_len=2, row_lo=1)
    # rejected before anything is launched
    add(hd=128, hq=5, hkv=2)
    for name, off in (("ldq", 4), ("ldk", 4), ("ldv", 4), ("ldo", 2)):
        for hd in (72, 128):
            add(hd=hd, q_len=2, causal=1, pre=1, ld_off={name: off})
    add(hd=128, q_len=129, causal=1, pre=1, head_stride=134 * 128)             # head-major: the encoder's kernel only
    add(hd=72, q_len=129, causal=1, pre=1, head_stride=134 * 72)
    # ---- ViT: hd 72, pre-scaled, hq == hkv, two segments
    for heads in (1, 8, 16):
        for seg in (64, 192) + tuple(VIT_ENDS):
            if heads != 8 and seg not in (64, 193, 448):
                continue
            for hint in (0, seg):
                for hm in (0, 1):
                    add(hd=72, pre=1, hq=heads, hkv=heads, cu=[0, seg, 2 * seg], hint=hint, head_major=hm)
    for hint in (0, 193):
        for hm in (0, 1):
            add(hd=72, pre=1, hq=8, hkv=8, cu=[0, 193, 449], hint=hint, head_major=hm)    # unequal: the hint does not hold
        add(hd=72, pre=1, hq=8, hkv=8, cu=[0, 193, 386], hint=hint, ldv_pad=8)            # ldk != ldv
    add(hd=72, pre=1, hq=8, hkv=8, cu=[0, 193, 386], head_major=1, ld_off={"ldk": 8})     # head-major needs ld = 72
    add(hd=72, pre=1, hq=8, hkv=8, cu=[0, 193, 386], head_major=1, ld_off={"ldq": 4})
    add(hd=72, pre=1, hq=8, hkv=8, cu=[0, 193, 386], ld_off={"ldo": 2})
    # ---- rows
    for rows in (1, 3, 16, 17):
        for slot in (0, 1):
            for nsplit in (0, 1, 127, 128):
                add(kind="rows", rows=rows, slot=slot, nsplit=nsplit)
    add(kind="rows", slot=1, slot_ld="small")
    add(kind="rows", ws="short")
    add(kind="rows", ws="absent")
    add(kind="rows", rows=17, ws="short")
    add(kind="rows", hq=34, hkv=2)
    add(kind="rows", hd=72)
    return out


def full(cell):
    return {**(ROWS_DEFAULTS if cell.get("kind") == "rows" else DEFAULTS), **cell}


def split_ws_bytes(parts, rows, hq, hd):
    return parts * rows * hq * (hd + 2) * 4


def query(cell):
    """every number of the cell's descriptor (the fields of cogs_attn_desc / cogs_attn_rows_desc that are not pointers)"""
    c = full(cell)
    if c["kind"] == "rows":
        kvd = c["hkv"] * c["hd"]
        nsplit = c["nsplit"] if c["nsplit"] > 1 else 1                      # cogs_attention_rows: nsplit <= 1 means 1
        need = split_ws_bytes(nsplit + 1, c["rows"], c["hq"], c["hd"])
        return dict(rows=c["rows"], hq=c["hq"], hkv=c["hkv"], head_dim=c["hd"], prefix_len=c["prefix_len"], tail_len=c["tail_len"],
                    ldq=(c["hq"] + 2 * c["hkv"]) * c["hd"], ldk=kvd, ldv=kvd, tail_ld=kvd, tail_row=c["tail_max"] * kvd,
                    nsplit_desc=c["nsplit"], nsplit=nsplit, has_slot=c["slot"],
                    tail_slot_ld=(c["tail_len"] - 1 if c["slot_ld"] == "small" else c["tail_max"]) if c["slot"] else 0,
                    has_ws=int(c["ws"] != "absent"), ws_alloc=need, ws_bytes={"exact": need, "short": need - 1, "absent": 0}[c["ws"]])
    hd, hq, hkv = c["hd"], c["hq"], c["hkv"]
    cu = c["cu"]
    q_len = cu[-1] if cu else c["q_len"]
    kv_len = q_len if cu else c["q_pos0"] + q_len
    if c["head_major"]:
        ld = dict(ldq=hd, ldk=hd, ldv=hd)
        head_stride = (q_len + GUARD_ROWS) * hd
    else:
        ld = dict(ldq=hq * hd + 8, ldk=hkv * hd + 8, ldv=hkv * hd + 8 + c["ldv_pad"])
        head_stride = c["head_stride"] or 0
    ld["ldo"] = hq * hd + 8
    for k, v in (c["ld_off"] or {}).items():
        ld[k] += v
    nsplit = c["nsplit"] if c["nsplit"] > 1 else 1                          # cogs_attention: nsplit <= 1 means 1
    need = split_ws_bytes(nsplit, q_len, hq, hd) if nsplit > 1 else 0
    has_ws = int(nsplit > 1 and c["ws"] != "absent")
    return dict(bf16=int(c["dtype"] == "bf16"), head_dim=hd, q_len=q_len, kv_len=kv_len, hq=hq, hkv=hkv, **ld, head_stride=head_stride,
                has_cu=int(cu is not None), has_row_lo=c["row_lo"], has_ws=has_ws, nseg=len(cu) - 1 if cu else 1,
                max_seqlen=max(b - a for a, b in zip(cu[:-1], cu[1:])) if cu else 0, uniform_seqlen=c["hint"], causal=c["causal"],
                q_pos0=c["q_pos0"], q_prescaled=c["pre"], force_rowwise=c["force_rowwise"], nsplit=nsplit, ws_alloc=need,
                ws_bytes=(need - 1 if c["ws"] == "short" else need) if has_ws else 0)


class Buffers:
    """zero-filled device buffers of the cell's size with GUARD_ROWS rows behind every matrix and a tracer-filled band around O;
    `desc` is the filled cogs_attn_desc / cogs_attn_rows_desc, `call()` runs it and returns the status after a synchronise,
    `guards_intact()` whether everything outside O's rows and columns kept its bits"""

    def __init__(self, cell, dev):
        import torch
        from cogstream_amd import _lib as L
        self.L, self.torch = L, torch
        c, q = full(cell), query(cell)
        self.rows_kind = c["kind"] == "rows"
        dt = torch.bfloat16 if c.get("dtype", "bf16") == "bf16" else torch.float32
        z = lambda n, t=dt: torch.zeros(n, dtype=t, device=dev)
        self.keep = []
        ws = None
        if q["has_ws"]:
            ws = z(q["ws_alloc"] // 4, torch.float32)
        if self.rows_kind:
            d = L.AttnRowsDesc()
            R = q["rows"]
            qb = z((R + GUARD_ROWS) * q["ldq"])
            kb, vb = z((q["prefix_len"] + GUARD_ROWS) * q["ldk"]), z((q["prefix_len"] + GUARD_ROWS) * q["ldv"])
            tk, tv = z((R + 1) * q["tail_row"]), z((R + 1) * q["tail_row"])
            self.o_rows, self.o_cols, self.ldo = R, q["hq"] * q["head_dim"], q["hq"] * q["head_dim"]
            d.dtype = L.dtype_code(dt)
            d.Q, d.ldq, d.K, d.V, d.ldk, d.ldv, d.prefix_len = qb.data_ptr(), q["ldq"], kb.data_ptr(), vb.data_ptr(), q["ldk"], q["ldv"], q["prefix_len"]
            d.tail_k, d.tail_v, d.tail_ld, d.tail_row_stride, d.tail_len = tk.data_ptr(), tv.data_ptr(), q["tail_ld"], q["tail_row"], q["tail_len"]
            d.rows, d.hq, d.hkv, d.head_dim, d.nsplit = R, q["hq"], q["hkv"], q["head_dim"], q["nsplit_desc"]
            if q["has_slot"]:
                slot = torch.arange(R, dtype=torch.int32, device=dev).repeat_interleave(c["tail_max"]).contiguous()   # row r reads slot r
                d.tail_slot, d.tail_slot_ld = slot.data_ptr(), q["tail_slot_ld"]
                self.keep.append(slot)
            self.keep += [qb, kb, vb, tk, tv]
            self.fn = L.lib.cogs_attention_rows
        else:
            d = L.AttnDesc()
            Lq, Lk, hd = q["q_len"], q["kv_len"], q["head_dim"]
            if c["head_major"]:
                hs = q["head_stride"]
                qb, kb, vb = z(q["hq"] * hs), z(q["hkv"] * hs), z(q["hkv"] * hs)
            else:
                qb, kb, vb = z((Lq + GUARD_ROWS) * q["ldq"]), z((Lk + GUARD_ROWS) * q["ldk"]), z((Lk + GUARD_ROWS) * q["ldv"])
            self.o_rows, self.o_cols, self.ldo = Lq, q["hq"] * hd, q["ldo"]
            d.dtype = L.dtype_code(dt)
            d.Q, d.K, d.V = qb.data_ptr(), kb.data_ptr(), vb.data_ptr()
            d.ldq, d.ldk, d.ldv, d.ldo, d.head_stride = q["ldq"], q["ldk"], q["ldv"], q["ldo"], q["head_stride"]
            if c["cu"]:
                cu = torch.tensor(c["cu"], dtype=torch.int32, device=dev)
                d.cu_seqlens = cu.data_ptr()
                self.keep.append(cu)
            d.nseg, d.max_seqlen = q["nseg"], q["max_seqlen"]
            if c["row_lo"]:                                                 # every row sees every key
                lo, hi = torch.zeros(Lq, dtype=torch.int32, device=dev), torch.full((Lq,), Lk, dtype=torch.int32, device=dev)
                d.row_lo, d.row_hi, d.bias = lo.data_ptr(), hi.data_ptr(), -1.0
                self.keep += [lo, hi]
            d.q_len, d.kv_len, d.hq, d.hkv, d.head_dim = Lq, Lk, q["hq"], q["hkv"], hd
            d.scale, d.causal, d.q_pos0 = 1.0 / hd ** 0.5, q["causal"], q["q_pos0"]
            d.force_rowwise, d.q_prescaled, d.nsplit = q["force_rowwise"], q["q_prescaled"], c["nsplit"]
            self.keep += [qb, kb, vb]
            self.fn = L.lib.cogs_attention
        if q["has_ws"]:
            d.ws = ws.data_ptr()
        d.ws_bytes = q["ws_bytes"]
        self.hint = 0 if self.rows_kind else q["uniform_seqlen"]
        fill = 0x7F7F if dt == torch.bfloat16 else 0x7F7F7F7F
        self.obuf = torch.full(((GUARD_ROWS + self.o_rows + GUARD_ROWS) * self.ldo,), fill,
                               dtype=torch.int16 if dt == torch.bfloat16 else torch.int32, device=dev)
        d.O = self.obuf.data_ptr() + GUARD_ROWS * self.ldo * self.obuf.element_size()
        self.fill, self.desc = fill, d
        self.keep.append(ws)

    def call(self):
        """(status, attn_last_kernel, attn_vit_last_end) of one call; a HIP error raises"""
        import ctypes as C
        L = self.L
        with L.debug_switch("attn_uniform_hint", self.hint):
            st = self.fn(L.current_stream(), C.byref(self.desc))
        self.torch.cuda.synchronize()
        if st == L.E_HIP:
            raise RuntimeError("cogs status E_HIP")
        return st, L.debug_get("attn_last_kernel"), L.debug_get("attn_vit_last_end")

    def guards_intact(self):
        o = self.obuf.view(-1, self.ldo)
        return bool((o[:GUARD_ROWS] == self.fill).all() and (o[GUARD_ROWS + self.o_rows:] == self.fill).all()
                    and (o[:, self.o_cols:] == self.fill).all())
