"""rsmi_crc_named_rows_dev under seeded random shapes, against test_named_rows.py's references:
random k and m, S up to 70 000, the three layouts with random phases, pitches and block strides,
random slots and folds, and entry arrays that mix named rows (repeats included) with every kind of
value that names nothing, at a random density.  Exact, like everything there."""
import numpy as np
import pytest

from test_named_rows import Halves, I32_MAX, I32_MIN, Outputs, assert_named, gpu, refs_of, set_folds  # noqa: F401

CASES = 40


def draw(rng, rsmi):
    k, m = int(rng.integers(1, 17)), int(rng.integers(1, 5))
    n = k + m
    S = int(rng.choice([rng.integers(1, 70001), rng.integers(1, 3000), 1024 * rng.integers(1, 65) + rng.integers(-1, 2)]))
    nb = int(rng.integers(1, 6))
    slots = int(rng.choice([1, 2, n, rng.integers(1, n + 1)]))
    layout = ["aligned", "ua", "halves"][int(rng.integers(0, 3))]
    if layout == "aligned":
        rs = rsmi.recommended_pitch(S) + 16 * int(rng.integers(0, 3))
        geo = (16 * int(rng.integers(0, 4)), rs, k * rs + 16 * int(rng.integers(0, 5)),
               16 * int(rng.integers(0, 4)), rs + 16, m * (rs + 16) + 16 * int(rng.integers(0, 5)))
    elif layout == "ua":
        geo = (int(rng.integers(0, 16)), S, k * S, int(rng.integers(0, 16)), S, m * S)
    else:
        drs, prs = S + int(rng.integers(0, 40)), S + int(rng.integers(0, 40))
        geo = (int(rng.integers(0, 32)), drs, k * drs + int(rng.integers(0, 40)),
               int(rng.integers(0, 32)), prs, m * prs + int(rng.integers(0, 40)))
    density = rng.choice([0.0, 0.1, 0.5, 1.0])
    junk = [-1, -2, n, n + 7, I32_MAX, I32_MIN, -n, 1 << 20]
    entries = np.where(rng.random((nb, slots)) < density, rng.integers(0, n, size=(nb, slots)),
                       rng.choice(junk, size=(nb, slots)))
    return k, m, S, nb, slots, geo, entries


@pytest.mark.gpu
def test_fuzz(gpu):
    torch, rsmi = gpu
    rng = np.random.default_rng(0x5EED0)
    codecs = {}
    try:
        for case in range(CASES):
            k, m, S, nb, slots, geo, entries = draw(rng, rsmi)
            shards = rng.integers(0, 256, size=(nb, k + m, S), dtype=np.uint8)
            fold16, fold32 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            outs = [(True, True), (True, False), (False, True)][int(rng.integers(0, 3))]
            c = codecs.setdefault((k, m), rsmi.Codec(k, m))
            c.set_option("crc16_fold", fold16)
            c.set_option("crc32_fold", fold32)
            ctx = (case, k, m, S, nb, slots, geo, fold16, fold32, outs)
            h = Halves(torch, shards, k, geo)
            d_rows = torch.from_numpy(entries.astype(np.int32)).cuda()
            out = Outputs(torch, nb * slots, *outs)
            h.call(c, d_rows.data_ptr(), slots, out, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ua = "" if h.aligned else ",UA"
            last = ("rs_crc32_named" + ("_mfma" if fold32 else "") if outs[1] else
                    "rs_crc16_named" + ("_mfma" if fold16 else "")) + "_kernel" + ua
            assert c.last_kernel() == last, (ctx, c.last_kernel())
            assert h.unchanged(), ctx
            r16, r32 = out.read((nb, slots))
            assert_named(rsmi, shards, entries, r16, r32, refs_of(shards), ctx)
    finally:
        for c in codecs.values():
            c.close()
