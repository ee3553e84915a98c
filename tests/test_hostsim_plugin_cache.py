"""The bookkeeping of the plug-in device cache (pydeseq2_amd/csrc/dsq_plugin_pool.h) on the host, over the fake device
allocator of tests/hostsim: LRU eviction under a byte budget, the free list, and entries that stay where they are while the
call that holds them runs - also when an allocation runs out of memory and evicts.  The memory pressure exists only inside
the fake."""
import numpy as np
import pytest

from tests import hostsim as hs

COUNTS, F64 = 0, 1
KB = 1024


def rounded(nbytes):
    return max(256, (nbytes + 255) // 256 * 256)


def accounting(pc, held=0):
    """resident / pooled agree with the entries and the free list; the fake device holds exactly those plus `held` bytes"""
    s = pc.state()
    ents = [pc.entry(e) for e in pc.entries()]
    assert s["entries"] == len(ents)
    assert s["resident"] == sum(e["cap"] + e["lists_cap"] for e in ents)
    assert s["pooled"] == sum(k for k, _ in pc.pool())
    assert s["live_bytes"] == s["resident"] + s["pooled"] + held
    assert s["bad_frees"] == 0
    return s


def put(pc, a, nbytes, kind=COUNTS):
    """a resident matrix with digest (a, a + 1) in a fresh buffer of nbytes"""
    buf = pc.take(nbytes)
    assert buf is not None
    return pc.insert(kind, 7, 11, a, a + 1, buf)


def test_held_entry_survives_an_out_of_memory_eviction():
    """The ADVICE scenario: a call holds the entry of its count matrix (with its mixed-design gene lists) while an allocation
    runs out of device memory and evicts an older entry.  The held pointer is still that entry, with the same digest, buffer
    and lists (with entries in a vector, the erase moved the held entry to another address)."""
    pc = hs.PluginPool(capacity=36 * KB, budget=1 << 20)
    pc.begin_call()
    old = put(pc, 100, 8 * KB)
    pc.begin_call()
    held = put(pc, 200, 8 * KB)
    pc.attach_lists(held, pc.take(2 * KB), n_rows=5, n_waves=6)
    spare = pc.take(4 * KB)
    pc.give(*spare)
    accounting(pc)
    before = pc.entry(held)
    assert pc.entries() == [old, held]
    # 22 KB live of 36: 20 KB more fit neither now nor once the free list went back; once `old` went back they do
    buf = pc.take(20 * KB)
    assert buf is not None and buf[1] == 20 * KB
    assert pc.entries() == [held]
    assert pc.entry(held) == before
    assert (before["a"], before["b"], before["n_rows"], before["n_waves"]) == (200, 201, 5, 6)
    s = accounting(pc, held=buf[1])
    assert s["evictions"] == 1 and s["pooled"] == 0
    # nothing untouched is left to evict: the allocation fails, the running call's entry stays
    assert pc.take(20 * KB) is None
    assert pc.entries() == [held] and pc.entry(held) == before
    pc.give(*buf)
    accounting(pc)
    pc.clear()
    assert accounting(pc)["live_bytes"] == 0


def test_forced_allocation_failures_evict_least_recently_used_first():
    pc = hs.PluginPool(capacity=1 << 20, budget=1 << 20)
    pc.begin_call()
    e = [put(pc, 10 * i, KB) for i in range(4)]
    pc.begin_call()
    assert pc.find(COUNTS, 7, 11, 0, 1) == e[0]  # touched by this call: not evictable now
    pc.fail_next(3)  # the first try, the retry after the free list went back, the retry after one eviction
    buf = pc.take(KB)
    assert buf is not None
    assert pc.entries() == [e[0], e[3]]  # e[1], then e[2]: least recently used first
    accounting(pc, held=buf[1])
    pc.give(*buf)
    accounting(pc)


def test_many_inserts_in_one_call_keep_earlier_pointers():
    pc = hs.PluginPool(capacity=1 << 24, budget=1 << 24)
    pc.begin_call()
    held = []
    for i in range(300):
        held.append(put(pc, 1000 + i, 256 * (1 + i % 5), kind=i % 2))
        assert pc.entries() == held
    for i, e in enumerate(held):
        x = pc.entry(e)
        assert (x["a"], x["b"], x["kind"], x["cap"]) == (1000 + i, 1001 + i, i % 2, 256 * (1 + i % 5))
    for i in (0, 17, 299):
        assert pc.find(i % 2, 7, 11, 1000 + i, 1001 + i) == held[i]
    accounting(pc)


def test_eviction_follows_least_recent_use_and_spares_the_running_call():
    pc = hs.PluginPool(capacity=1 << 20, budget=3 * KB)
    pc.begin_call()
    a, b, c = (put(pc, x, KB) for x in (1, 2, 3))
    pc.begin_call()
    assert pc.find(COUNTS, 7, 11, 1, 2) == a
    d = put(pc, 4, KB)  # b is the least recently used entry this call has not touched
    assert pc.entries() == [a, c, d]
    e = put(pc, 5, KB)
    assert pc.entries() == [a, d, e]
    f = put(pc, 6, KB)  # everything resident is this call's: over budget until the call ends
    assert pc.entries() == [a, d, e, f]
    s = accounting(pc)
    assert s["resident"] == 4 * KB > s["budget"] and s["evictions"] == 2
    pc.begin_call()
    assert pc.entries() == [d, e, f]  # a was touched first in the last call: least recently used
    s = accounting(pc)
    assert s["resident"] <= s["budget"] and s["evictions"] == 3


def test_budget_smaller_than_one_matrix():
    pc = hs.PluginPool(capacity=1 << 20, budget=512)
    pc.begin_call()
    x = put(pc, 1, 2 * KB)
    y = put(pc, 2, 2 * KB)
    assert pc.entries() == [x, y]  # the running call's entries survive it
    accounting(pc)
    pc.begin_call()
    s = accounting(pc)
    assert pc.entries() == [] and s["resident"] == 0 and s["evictions"] == 2
    assert s["pooled"] <= s["budget"]


def test_disabled_cache_drops_everything_at_begin_call():
    pc = hs.PluginPool(capacity=1 << 20, budget=1 << 20, enabled=False)
    pc.begin_call()
    x = put(pc, 1, 2 * KB)
    pc.attach_lists(x, pc.take(KB), 1, 2)
    put(pc, 2, 3 * KB, kind=F64)
    assert accounting(pc)["resident"] == 6 * KB
    pc.begin_call()
    s = accounting(pc)
    assert pc.entries() == [] and s["resident"] == 0 and s["evictions"] == 0
    assert sorted(k for k, _ in pc.pool()) == [KB, 2 * KB, 3 * KB]  # (their buffers went to the free list)


def test_requests_round_up_to_256_bytes():
    pc = hs.PluginPool(capacity=1 << 20, budget=1 << 20)
    for n, cap in [(0, 256), (1, 256), (256, 256), (257, 512), (1000, 1024), (4097, 4352)]:
        buf = pc.take(n)
        assert buf[1] == cap == rounded(n)
        pc.give(*buf)
        pc.clear()
    assert accounting(pc)["live_bytes"] == 0


def test_free_list_reuse_matches_the_rule():
    """A pooled buffer of k bytes serves a request of `bytes` (rounded) only when bytes <= k <= 2 * bytes + 4096, the smallest
    such buffer first (the first of equal ones in list order); otherwise the request is a fresh allocation."""
    rng = np.random.default_rng(5)
    for trial in range(40):
        pc = hs.PluginPool(capacity=1 << 26, budget=1 << 26)
        for _ in range(int(rng.integers(0, 10))):
            pc.give(*pc.take(int(rng.integers(1, 40 * KB))))
        held = 0
        for _ in range(20):
            want = int(rng.integers(0, 40 * KB))
            r = rounded(want)
            pool = pc.pool()
            fit = [i for i, (k, _) in enumerate(pool) if r <= k <= 2 * r + 4096]
            mallocs = pc.state()["mallocs"]
            p, cap = pc.take(want)
            if fit:
                best = min(fit, key=lambda i: (pool[i][0], i))
                assert (cap, p) == pool[best]
                assert pc.state()["mallocs"] == mallocs
            else:
                assert cap == r and p not in [q for _, q in pool]
                assert pc.state()["mallocs"] == mallocs + 1
            held += cap
            accounting(pc, held)
        pc.clear()


def test_give_trims_the_largest_pooled_buffers_over_budget():
    pc = hs.PluginPool(capacity=1 << 20, budget=8 * KB)
    pc.begin_call()
    put(pc, 1, 2 * KB)
    bufs = [pc.take(n) for n in (KB, 4 * KB, 2 * KB, 2 * KB)]
    held = sum(b[1] for b in bufs)
    for b, pooled in zip(bufs, ([KB], [KB, 4 * KB], [KB, 2 * KB], [KB, 2 * KB, 2 * KB])):
        pc.give(*b)
        held -= b[1]
        assert [k for k, _ in pc.pool()] == pooled
        s = accounting(pc, held)
        assert s["pooled"] + s["resident"] <= s["budget"]


def test_accounting_holds_after_every_operation():
    """Random calls of every operation, failed allocations and budget changes included; the bookkeeping is checked after
    each one, and every entry the running call holds must still be there, unchanged."""
    rng = np.random.default_rng(11)
    pc = hs.PluginPool(capacity=96 * KB, budget=48 * KB)
    held_bufs, call = [], {}
    next_digest = 1
    for step in range(3000):
        op = int(rng.integers(0, 9))
        if op == 0:
            pc.begin_call()
            call = {}
        elif op == 1:
            buf = pc.take(int(rng.integers(0, 12 * KB)))
            if buf is not None:
                held_bufs.append(buf)
        elif op == 2 and held_bufs:
            pc.give(*held_bufs.pop(int(rng.integers(0, len(held_bufs)))))
        elif op == 3 and held_bufs:
            buf = held_bufs.pop(int(rng.integers(0, len(held_bufs))))
            e = pc.insert(COUNTS, 7, 11, next_digest, next_digest + 1, buf)
            call[e] = pc.entry(e)
            next_digest += 2
        elif op == 4 and pc.entries():
            x = pc.entry(pc.entries()[int(rng.integers(0, len(pc.entries())))])
            e = pc.find(x["kind"], x["N"], x["G"], x["a"], x["b"])
            call[e] = pc.entry(e)
        elif op == 5 and call:
            e = list(call)[int(rng.integers(0, len(call)))]
            if call[e]["d_lists"] == 0:
                buf = pc.take(int(rng.integers(1, 2 * KB)))
                if buf is not None:
                    pc.attach_lists(e, buf, 3, 4)
                    call[e] = pc.entry(e)
        elif op == 6:
            pc.fail_next(int(rng.integers(1, 4)))
        elif op == 7:
            pc.set_budget(int(rng.integers(4, 64)) * KB)
        elif op == 8 and rng.random() < 0.05:
            pc.clear()
            call = {}
        ents = pc.entries()
        for e, x in call.items():
            assert e in ents and pc.entry(e) == x, step
        accounting(pc, sum(b[1] for b in held_bufs))
    pc.fail_next(0)
    for b in held_bufs:
        pc.give(*b)
    pc.clear()
    s = accounting(pc)
    assert s["live_bytes"] == 0 and s["live_blocks"] == 0 and s["resident"] == 0 and s["pooled"] == 0


@pytest.fixture(autouse=True)
def _fresh_pool():
    yield
    hs.PluginPool(capacity=0, budget=0)  # (frees whatever a failed test left)
