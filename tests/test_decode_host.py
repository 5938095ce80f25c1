"""cogstream_amd/decode.py without a GPU: the three row steppers, the token history and the one token loop against a toy CPU
engine whose logits are an exact, integer-valued function of the ordered (position, token) history -- read back from the K / V
rows the stepper is responsible for (the cache rows behind the prompt for SingleRow and Replay, the tails through the slot
table for Lockstep). A wrong row, slot, parent, position or stale copy changes the logits; "equal" is torch.equal."""
from types import SimpleNamespace

import pytest
import torch

from cogstream_amd import _lib as L
from cogstream_amd import decode

LAYERS, KVD, VOCAB, ROWS, STEPS = 2, 4, 16, 3, 6
PROMPT = [5, 9, 2]
P = len(PROMPT)
# identity, a permutation, a duplicated parent, all rows from one parent, another permutation, identity
PARENTS = [(0, 1, 2), (2, 0, 1), (0, 0, 2), (1, 1, 1), (1, 2, 0), (0, 1, 2)]
TOKENS = [(3, 7, 11), (1, 4, 13), (8, 2, 6), (15, 10, 0), (12, 5, 9), (14, 3, 7)]
MOD = 65521


def kv_row(layer, pos, tok):
    """the K and V row the toy writes for `tok` at position `pos` in `layer`"""
    return [pos, tok, layer, (pos * tok) % 7], [tok + 1, pos + 3, 2 * layer + 1, (pos + tok) % 5]


def logits_of(acc):
    return torch.tensor([float((acc * (v + 3) + v * v) % 1009) for v in range(VOCAB)])


def evaluate(history):
    """direct evaluation: the logits after the ordered token `history` (prompt included)"""
    acc = 0
    for layer in range(LAYERS):
        for pos, tok in enumerate(history):
            k, v = kv_row(layer, pos, tok)
            for x in k + v:
                acc = (acc * 31 + x + 1) % MOD
    return logits_of(acc)


def read_back(k, v):
    """the same function of K / V rows [layers, n, kv_dim] as they are found"""
    acc = 0
    for layer in range(LAYERS):
        for j in range(k.shape[1]):
            for x in k[layer, j].tolist() + v[layer, j].tolist():
                acc = (acc * 31 + int(x) + 1) % MOD
    return logits_of(acc)


class ToyCache:
    def __init__(self, max_len):
        self.k = torch.full((LAYERS, max_len, KVD), -1.0)
        self.v = torch.full((LAYERS, max_len, KVD), -1.0)
        self.len = 0

    def reset(self, length=0):
        self.len = length


class Toy:
    """the members decode.py needs of an engine; the embedding of a token is its id"""

    def __init__(self, dtype=torch.float32, head_dim=KVD):
        self.cfg = SimpleNamespace(vocab_size=VOCAB, head_dim=head_dim, num_hidden_layers=LAYERS)
        self.dtype, self.device, self.forwards = dtype, torch.device("cpu"), 0

    def embed_tokens(self, ids):
        return ids.reshape(-1).to(torch.float32).view(-1, 1)

    @staticmethod
    def _write(k, v, pos, tok):
        for layer in range(LAYERS):
            kr, vr = kv_row(layer, pos, tok)
            k[layer], v[layer] = torch.tensor(kr, dtype=k.dtype), torch.tensor(vr, dtype=v.dtype)

    def forward(self, embeds, cache):
        self.forwards += 1
        for e in embeds.reshape(-1).tolist():
            self._write(cache.k[:, cache.len], cache.v[:, cache.len], cache.len, int(e))
            cache.reset(cache.len + 1)
        return {"logits": read_back(cache.k[:, :cache.len], cache.v[:, :cache.len])}

    def new_rows_kv(self, cache, n_rows, tail_max, slots=False):
        tk = torch.full((LAYERS, n_rows, tail_max, KVD), -1.0)
        tv = torch.full((LAYERS, n_rows, tail_max, KVD), -1.0)
        kv = SimpleNamespace(cache=cache, prefix_len=cache.len, tail_k=tk, tail_v=tv, tail_max=tail_max, tail_len=0)
        if slots:
            return kv, tk, tv, torch.zeros(n_rows, tail_max, dtype=torch.int32)
        return kv, tk, tv

    def decode_rows(self, embeds, kv, tail_slot=None):
        t, n = kv.tail_len, kv.prefix_len
        toks = [int(e) for e in embeds.reshape(-1).tolist()]
        for r, tok in enumerate(toks):
            self._write(kv.tail_k[:, r, t], kv.tail_v[:, r, t], n + t, tok)
        out = torch.empty(len(toks), VOCAB)
        for r in range(len(toks)):
            slot = [int(tail_slot[r, j]) if tail_slot is not None else r for j in range(t + 1)]
            k = torch.cat([kv.cache.k[:, :n]] + [kv.tail_k[:, s, j].unsqueeze(1) for j, s in enumerate(slot)], 1)
            v = torch.cat([kv.cache.v[:, :n]] + [kv.tail_v[:, s, j].unsqueeze(1) for j, s in enumerate(slot)], 1)
            out[r] = read_back(k, v)
        kv.tail_len = t + 1
        return out


def prefilled(eng, room=STEPS):
    cache = ToyCache(P + room + 1)
    first = eng.forward(eng.embed_tokens(torch.tensor(PROMPT)), cache)["logits"]
    assert torch.equal(first, evaluate(PROMPT)) and cache.len == P
    return cache, first


def ancestry(schedule):
    """the token history of every row after each step of `schedule` = [(parents | None, tokens)]"""
    rows, out = [[] for _ in range(ROWS)], []
    for parents, tokens in schedule:
        rows = [rows[parents[r] if parents is not None else r] + [tokens[r]] for r in range(ROWS)]
        out.append(rows)
    return out


def run_schedule(stepper, with_parents):
    schedule = [(PARENTS[s] if with_parents else None, TOKENS[s]) for s in range(STEPS)]
    got = []
    for (parents, tokens), rows in zip(schedule, ancestry(schedule)):
        par = torch.tensor(parents, dtype=torch.int64) if parents is not None else None
        logits = stepper.step(torch.tensor(tokens, dtype=torch.int64), par)
        assert len(logits) == ROWS and all(l.shape == (VOCAB,) and l.dtype == torch.float32 for l in logits)
        assert torch.is_tensor(logits) or (parents is None and isinstance(stepper, decode.Replay))
        for r in range(ROWS):
            assert torch.equal(logits[r], evaluate(PROMPT + rows[r])), (parents, r)
        got.append([l.clone() for l in logits])
    return got


@pytest.mark.parametrize("kind", ["replay", "table", "gather"])
def test_steppers_follow_parents(kind):
    eng = Toy()
    cache, _ = prefilled(eng)
    before = cache.k[:, :P].clone(), cache.v[:, :P].clone()
    with L.debug_switch("beam_gather_tails", int(kind == "gather")):
        st = decode.Replay(eng, cache, ROWS, STEPS) if kind == "replay" else decode.Lockstep(eng, cache, ROWS, STEPS, slots=True)
        assert kind == "replay" or st.gather == (kind == "gather")
        got = run_schedule(st, True)
    if kind != "replay":           # table and gather give identical logits
        cache2, _ = prefilled(eng)
        with L.debug_switch("beam_gather_tails", int(kind != "gather")):
            other = run_schedule(decode.Lockstep(eng, cache2, ROWS, STEPS, slots=True), True)
        assert all(torch.equal(a, b) for x, y in zip(got, other) for a, b in zip(x, y))
    st.close()
    assert cache.len == P and torch.equal(cache.k[:, :P], before[0]) and torch.equal(cache.v[:, :P], before[1])


@pytest.mark.parametrize("kind", ["replay", "lockstep"])
def test_plain_rows(kind):
    eng = Toy()
    cache, _ = prefilled(eng)
    before = cache.k[:, :P].clone(), cache.v[:, :P].clone()
    st = decode.Replay(eng, cache, ROWS, STEPS) if kind == "replay" else decode.Lockstep(eng, cache, ROWS, STEPS)
    run_schedule(st, False)
    st.close()
    assert cache.len == P and torch.equal(cache.k[:, :P], before[0]) and torch.equal(cache.v[:, :P], before[1])


def test_rows_stepper_rule():
    for dtype, hd, want in ((torch.bfloat16, 128, decode.Lockstep), (torch.float32, 128, decode.Replay),
                            (torch.bfloat16, 64, decode.Replay)):
        eng = Toy(dtype, hd)
        cache, _ = prefilled(eng)
        assert type(decode.rows_stepper(eng, cache, ROWS, STEPS, slots=True)) is want


def test_replay_steps_only_live_rows():
    eng = Toy()
    cache, _ = prefilled(eng)
    st = decode.Replay(eng, cache, ROWS, STEPS)
    st.k.fill_(-7.0)
    st.v.fill_(-7.0)
    lives = [[0, 1, 2], [0, 1, 2], [0, 2], [0, 2], [2], [2]]
    rows = ancestry([(None, TOKENS[s]) for s in range(STEPS)])
    for s, live in enumerate(lives):
        logits = st.step(torch.tensor(TOKENS[s], dtype=torch.int64), live=live)
        for r in range(ROWS):
            if r in live:
                assert torch.equal(logits[r], evaluate(PROMPT + rows[s][r])), (s, r)
            else:                  # the private copies of rows no longer live are not written
                assert logits[r] is None and bool((st.k[r, :, s] == -7.0).all()) and bool((st.v[r, :, s] == -7.0).all()), (s, r)
    st.close()
    assert cache.len == P


def test_single_row_and_close():
    for n_kept, want_len in ((2, P + 1), (STEPS, P + STEPS - 1)):       # an early stop; the full run
        eng = Toy()
        cache, _ = prefilled(eng)
        st = decode.SingleRow(eng, cache, P)
        toks = [t[0] for t in TOKENS]
        for s in range(STEPS - 1):                                      # STEPS tokens: the first from the prompt's logits
            logits = st.step(torch.tensor(toks[s:s + 1]))
            assert logits.shape == (1, VOCAB) and torch.equal(logits[0], evaluate(PROMPT + toks[:s + 1]))
        assert cache.len == P + STEPS - 1
        st.close(n_kept)
        assert cache.len == want_len


def test_history_follows_parents(monkeypatch):
    calls = []
    monkeypatch.setattr(decode.ops, "logits_process",
                        lambda logits, prev, pen, allowed, temp: calls.append((None if prev is None else prev.tolist(), pen, allowed, temp)))
    eng = Toy()
    prompt_ids = torch.tensor([[21, 22, 23, 24]])
    hist = decode.History(eng, ROWS, STEPS, prompt_ids, 1.05, [1, 2, 3], alloc=torch.zeros)
    assert hist.on and hist.toks.shape == (ROWS, STEPS) and hist.allowed.tolist() == [1, 2, 3] and hist.allowed.dtype == torch.int32
    row = torch.zeros(VOCAB)
    hist.process(row, 0, 0)
    assert calls.pop() == ([21, 22, 23, 24], 1.05, hist.allowed, 1.0)
    rows = ancestry(list(zip(PARENTS, TOKENS)))
    for s in range(STEPS):
        hist.reorder(torch.tensor(PARENTS[s], dtype=torch.int64))
        hist.toks[:, s] = torch.tensor(TOKENS[s], dtype=torch.int64)
        for r in range(ROWS):
            hist.process(row, r, s + 1)
            assert calls.pop() == ([21, 22, 23, 24] + rows[s][r], 1.05, hist.allowed, 1.0), (s, r)
    assert hist.toks.tolist() == rows[-1]
    # penalty off, mask on: no history is handed over; both off: the processor is not called; no prompt ids, no tokens: None
    hist = decode.History(eng, 1, STEPS, prompt_ids, 1.0, [4])
    hist.process(row, 0, 0)
    assert calls.pop() == (None, 1.0, hist.allowed, 1.0)
    hist = decode.History(eng, 1, STEPS, None, 1.0, None)
    hist.process(row, 0, 3)
    assert not hist.on and not calls
    hist = decode.History(eng, 1, STEPS, None, 1.3, None)
    hist.process(row, 0, 0)
    assert calls.pop() == (None, 1.3, None, 1.0)
    hist.toks[0, 0] = 6
    hist.process(row, 0, 1)
    assert calls.pop() == ([6], 1.3, None, 1.0)


def test_host_draw_block_of_one_row_is_the_single_row_draw():
    """the [vocab] draw of the former single-row loop: torch.empty(V).exponential_(1, generator=g)"""
    for seed in (0, 1, 2):
        g1, g2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        want = torch.empty(VOCAB, dtype=torch.float32).exponential_(1, generator=g1)
        assert torch.equal(decode.host_draw_block(g2, 1, VOCAB)[0], want)
        assert torch.equal(g1.get_state(), g2.get_state())


# ------------------------------------------------------------------------------------------------- the token loop
NEW = 10            # crosses the 8-step stop test of the device sampler


def _stub_draws(monkeypatch):
    """argmax as it is; "sampling" = (argmax + Philox offset + seed + the first of the row's host draws) mod V: the loop's
    offsets and draw rows decide the tokens. Both consume the logits row they are given, as a sampler may; the processors are
    counted (what they are handed is test_history_follows_parents's)"""
    calls = []

    def argmax(logits, out):
        out.copy_(logits.argmax().reshape(1))
        logits.fill_(-1.0)

    def sample(logits, top_k, top_p, draws=None, seed=0, offset=0, temperature=1.0, out=None):
        assert draws is None or draws.shape == (VOCAB,)
        extra = int(draws[0].item() * 1000) if draws is not None else 0
        out.copy_(((logits.argmax() + offset + seed + extra) % VOCAB).reshape(1))
        logits.fill_(-1.0)

    monkeypatch.setattr(decode.ops, "argmax", argmax)
    monkeypatch.setattr(decode.ops, "sample", sample)
    monkeypatch.setattr(decode.ops, "logits_process", lambda logits, *a: calls.append(logits))
    return calls


def _free_run(n_rows, do_sample, seed=0, host_seed=None):
    """the tokens without a stop, straight from evaluate(); host_seed: the host sampler's generator"""
    g = torch.Generator().manual_seed(host_seed) if host_seed is not None else None
    rows = [[] for _ in range(n_rows)]
    for s in range(NEW):
        block = decode.host_draw_block(g, n_rows, VOCAB) if g is not None else None
        for r, toks in enumerate(rows):
            a = int(evaluate(PROMPT + toks).argmax())
            extra = int(block[r, 0].item() * 1000) if g is not None else 0
            toks.append((a + decode.philox_offset(s, n_rows, r) + seed + extra) % VOCAB if do_sample else a)
    return rows


def _generator_after(steps, n_rows, host_seed):
    g = torch.Generator().manual_seed(host_seed)
    for _ in range(steps):
        decode.host_draw_block(g, n_rows, VOCAB)
    return g.get_state()


def _loop(eng, n_rows, cache=None, first=None, **kw):
    if cache is None:
        cache, first = prefilled(eng, NEW)
    args = dict(max_new_tokens=NEW, eos_token_id=(), ignore_eos=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0,
                repetition_penalty=1.0, allowed_ids=None, prompt_ids=None, generator=None, sampler="device", seed=0)
    args.update(kw)
    return decode.sample(eng, first, cache, P, n_rows, **args), cache


def test_loop_single_row(monkeypatch):
    _stub_draws(monkeypatch)
    eng = Toy()
    free = _free_run(1, False)
    got, cache = _loop(eng, 1)
    assert got == free and cache.len == P + NEW - 1
    for hit in (2, 8):                          # a stop inside the first 8-step window, one in the second
        eos = free[0][hit]
        want = decode.truncate_at_eos(free, [eos])
        got, cache = _loop(eng, 1, eos_token_id=[eos])
        assert got == want and cache.len == P + len(want[0]) - 1
        got, cache = _loop(eng, 1, eos_token_id=[eos], ignore_eos=True)
        assert got == free and cache.len == P + NEW - 1
    assert _loop(eng, 1, max_new_tokens=1)[0] == [free[0][:1]]
    got, cache = _loop(eng, 1, max_new_tokens=0)
    assert got == [[]] and cache.len == P
    sampled = _free_run(1, True, seed=5)
    assert _loop(eng, 1, do_sample=True, seed=5)[0] == sampled
    # host sampler: one [V] draw per issued step, none past the stop
    free = _free_run(1, True, host_seed=7)
    for eos_ids in ([], [free[0][2]]):
        want = decode.truncate_at_eos(free, eos_ids)
        g = torch.Generator().manual_seed(7)
        got, cache = _loop(eng, 1, do_sample=True, sampler="host", generator=g, seed=None, eos_token_id=eos_ids)
        assert got == want and cache.len == P + len(want[0]) - 1
        assert torch.equal(g.get_state(), _generator_after(len(want[0]), 1, 7))
    # seed=None, device sampler: one randint draw
    g, ref = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=ref).item())
    assert _loop(eng, 1, do_sample=True, generator=g, seed=None)[0] == _free_run(1, True, seed=seed)
    assert torch.equal(g.get_state(), ref.get_state())


def test_loop_runs_the_processors_on_the_prompt_row(monkeypatch):
    """N > 1: the one prefill row is processed once, in place, also when nothing is generated; N = 1: only when a token is"""
    calls = _stub_draws(monkeypatch)
    eng = Toy()
    for n_rows, new, want in ((ROWS, 0, 1), (1, 0, 0), (ROWS, 1, 1), (1, 1, 1), (1, 3, 3), (ROWS, 3, 1 + 2 * ROWS)):
        del calls[:]
        cache, first = prefilled(eng, NEW)
        _loop(eng, n_rows, cache, first, do_sample=n_rows > 1, allowed_ids=[1, 2], max_new_tokens=new)
        assert len(calls) == want and (not calls or calls[0] is first), (n_rows, new)


@pytest.mark.parametrize("kind", ["replay", "lockstep"])
def test_loop_rows(monkeypatch, kind):
    _stub_draws(monkeypatch)
    eng = Toy() if kind == "replay" else Toy(torch.bfloat16, 128)
    free = _free_run(ROWS, True, seed=3)
    got, cache = _loop(eng, ROWS, do_sample=True, seed=3)
    assert got == free and cache.len == P
    eos = free[0][2]
    want = decode.truncate_at_eos(free, [eos])
    got, cache = _loop(eng, ROWS, do_sample=True, seed=3, eos_token_id=[eos])
    assert got == want and cache.len == P
    assert _loop(eng, ROWS, do_sample=True, seed=3, max_new_tokens=1)[0] == [r[:1] for r in free]
    assert _loop(eng, ROWS, do_sample=True, seed=3, max_new_tokens=0)[0] == [[], [], []]
    # host sampler: one [rows, V] block per issued step, none past the stop. Row 0 stops at its first token, the others at their
    # second at the latest: a per-row stepper steps a finished row no further (one forward per kept token after the first)
    free0 = _free_run(ROWS, True, host_seed=7)
    for eos_ids in ([], sorted({free0[0][0]} | {r[1] for r in free0[1:]})):
        want = decode.truncate_at_eos(free0, eos_ids)
        assert not eos_ids or len({len(r) for r in want}) > 1
        g = torch.Generator().manual_seed(7)
        eng.forwards = 0
        got, cache = _loop(eng, ROWS, do_sample=True, sampler="host", generator=g, seed=None, eos_token_id=eos_ids)
        assert got == want and cache.len == P
        assert torch.equal(g.get_state(), _generator_after(max(len(r) for r in want), ROWS, 7))
        if kind == "replay":
            assert eng.forwards == 1 + sum(len(r) - 1 for r in want)        # the prompt pass + the steps
    g, ref = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=ref).item())
    got, _ = _loop(eng, ROWS, do_sample=True, generator=g, seed=None)
    assert got == _free_run(ROWS, True, seed=seed) and torch.equal(g.get_state(), ref.get_state())
