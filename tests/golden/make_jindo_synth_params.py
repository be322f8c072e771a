"""Generate tests/golden/jindo_synth_params.json: Jindo parameter sets that NewParameters never
produces but rg_jindo_create accepts (include/ringo.h: any power-of-two d in 2..1024, up to four
NTT-friendly ring primes below 2^62 per ring, any base below 2^32).

jindo_params.json restates NewParameters: d = 256, at most three ring primes of one bit size
below 2^61, base 12640..60272.  The sets here are hand-chosen to reach the kernels and branches
that corner never runs (the `reaches` field of each set; DESIGN.md has the table).  They have the
keys of jindo_params.json that describe a shape, so jindo.Parameters.from_dict and
coracle.CJindo take them unchanged; they have no target_n, no sampler widths and no norm bounds
(they are used with injected randomness only, and the tests derive the norm bounds from each
proof's exact norms).

Derived: rank = (rows - 1) cols slots, in_com_dcmp_len = (cols + 1) in_msis, batch = 1.
Ring primes: for a requested bit count b, the smallest primes p = 1 mod 2d with p > 2^b, in
increasing order (consecutive ones where a ring asks twice for one size); a negative count -b
asks for the largest such primes below 2^b, in decreasing order.  The qo primes are chosen the
same way, skipping any prime already in q.  Only pyref.is_prime is used, so anyone can reproduce
them.  The field moduli come from fields.json.  Running the script rewrites the JSON byte for
byte.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import pyref  # noqa: E402


def pick_primes(bit_counts, d, used):
    """One prime per entry of bit_counts (see the module docstring), none of them in `used`."""
    out, taken = [], set(used)
    for b in bit_counts:
        step = 2 * d
        if b > 0:
            p = ((1 << b) // step + 1) * step + 1
        else:
            p = (((1 << -b) - 2) // step) * step + 1
        while p in taken or not pyref.is_prime(p):
            p += step if b > 0 else -step
        assert (p > 1 << b) if b > 0 else (p < 1 << -b)
        taken.add(p)
        out.append(p)
    return out


# name, field, base, exp, d, slots, rows, cols, in_msis, out_msis, mlwe, q bits, qo bits,
# log_in_cut, log_out_cut, what it reaches
SPECS = [
    ("syn_d128_q2", "jindo_zp", 60272, 16, 128, 8, 5, 2, 3, 2, 3, [45, 45], [40], 20, 10,
     "prep_kernel, round_kernel (2->1 limbs, 1->2 in the verifier's lift), norm/decode at d = 128"),
    ("syn_d128_mixed4", "jindo_zp", 60272, 16, 128, 8, 5, 2, 2, 2, 3, [60, 31, 45, 61], [50, 50, 33], 30, 25,
     "4-limb Garner with unequal primes (the % q_j arm), a 4-word CRT value"),
    ("syn_d256_q62", "jindo_zp", 60272, 16, 256, 16, 5, 2, 2, 2, 3, [61, 61], [61], 20, 10,
     "primes in (2^61, 2^62): prep_kernel at d = 256, round256_kernel at its limit, the MFMA MAC with 8 digits"),
    ("syn_d64", "jindo_zp", 60272, 16, 64, 4, 5, 2, 2, 2, 3, [40, 40], [40, 40], 20, 10,
     "one-wave-sized polynomials under 256-thread workgroups"),
    ("syn_d8_p63", "p63", 47104, 4, 8, 2, 3, 1, 2, 2, 2, [40, 40], [40], 20, 10,
     "d % 16 != 0: generic MAC; d far below the workgroup"),
    ("syn_d1024_mult", "mult_zp", 60256, 8, 1024, 128, 3, 1, 2, 2, 2, [50, 50], [50], 20, 10,
     "kMaxD: largest static / dynamic LDS of prep, round, norm, decode"),
    ("syn_b70001_p63", "p63", 70001, 4, 256, 64, 3, 1, 2, 2, 2, [50, 50], [50], 20, 10,
     "base >= 2^16: b2 == 0, one digit per division"),
    ("syn_b7000_e5_p63", "p63", 7000, 5, 256, 48, 3, 1, 2, 2, 2, [50, 50], [50], 20, 10,
     "odd exp in the pair loop; slots * exp = 240 < d (digit coefficients no thread writes)"),
    ("syn_b251_e32_jindo", "jindo_zp", 251, 32, 256, 8, 3, 1, 2, 2, 2, [50, 50], [50], 20, 10,
     "L = 4 off dc_digits (general loop); slow b2 path"),
    # with the smallest primes above 2^61, syn_d256_q62's inner product
    # (8 terms) stays below the WIDE threshold 2 log2(q - 1) + log2(T + 1) >= 127.5 and inside the
    # MFMA MAC's bound; 12 terms of primes just below 2^62 cross both
    ("syn_d256_q62top", "jindo_zp", 60272, 16, 256, 16, 5, 2, 2, 2, 7, [-62, -62], [-62], 20, 10,
     "largest primes below 2^62 and 12 inner terms: mac_kernel<.., WIDE> (third accumulator word)"),
]


def main(out):
    fields = json.load(open(os.path.join(HERE, "fields.json")))
    sets = {}
    for (name, field, base, exp, d, slots, rows, cols, in_msis, out_msis, mlwe, qb, qob, cin, cout, reaches) in SPECS:
        q = pick_primes(qb, d, [])
        qo = pick_primes(qob, d, q)
        assert slots * exp <= d and len(qo) <= len(q) and min(q + qo) > base
        sets[name] = {
            "batch": 1, "rank": (rows - 1) * cols * slots, "rows": rows, "cols": cols, "base": base, "exp": exp,
            "slots": slots, "d": d, "in_msis": in_msis, "out_msis": out_msis, "mlwe": mlwe, "log_in_cut": cin,
            "log_out_cut": cout, "in_com_dcmp_len": (cols + 1) * in_msis, "q": q, "qo": qo,
            "field_q_hex": fields[field]["q_hex"], "field": field, "reaches": reaches}
    with open(out, "w") as f:
        json.dump(sets, f, indent=1)
        f.write("\n")
    print("wrote", out, list(sets))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "jindo_synth_params.json"))
