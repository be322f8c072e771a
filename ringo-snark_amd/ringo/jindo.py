"""jindo mirror (jindo/) over libringo.

    params = Parameters(...)            # shapes as jindo.Parameters holds them (params.go:64-123)
    prv = NewProver(params, b"Jindo!")  # prover.go:28 (commit key derived from the CRS on the host)
    com, open_ = prv.Commit(v, rnd)     # prover.go:45, randomness injected (see Randomness)

The reference's Commit draws its randomness internally (crypto/rand, Gaussian samplers); this
mirror takes those draws as arguments so the result is bit-exact against Go given identical
draws.  The Go-side NewParameters float search is not re-derived here: shapes
are passed in (tests take them from committed fixtures).
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import JindoParamsC, JindoSeedsC, JindoStddevsC, check, iptr, lib, ptr, vp
from .bigpoly import RingoPanic, _addr, _stream


STDDEV_KEYS = ("ecd_sd", "ecd_blind_sd", "mask_sd", "mask_blind_sd", "mlwe_sd", "mask_mlwe_sd")


@dataclass
class Seeds:
    """One 32-byte seed per sampler Commit draws from (include/ringo.h rg_jindo_seeds)."""
    enc_cdt: bytes
    enc_cosac: bytes
    enc_cosac_round: bytes
    mlwe_cdt: bytes
    mlwe_round: bytes
    uniform: bytes

    @classmethod
    def derive(cls, master):
        """Six seeds from one: SHA-256(master || name) (a convenience; Go draws each from crypto/rand)."""
        import hashlib
        return cls(**{k: hashlib.sha256(bytes(master) + k.encode()).digest() for k in cls.__dataclass_fields__})

    def raw(self):
        return b"".join(getattr(self, k) for k in self.__dataclass_fields__)

    def c_struct(self):
        s = JindoSeedsC()
        for k in self.__dataclass_fields__:
            v = getattr(self, k)
            if len(v) != 32:
                raise RingoPanic("seed must be 32 bytes")
            ctypes.memmove(getattr(s, k), v, 32)
        return s


@dataclass
class Parameters:
    rank: int
    rows: int
    cols: int
    slots: int
    exp: int
    d: int
    in_msis: int
    out_msis: int
    mlwe: int
    dcmp: int
    log_in_cut: int
    log_out_cut: int
    base: int
    q: list
    qo: list
    field_q: int
    stddevs: tuple = None  # ecd, ecd_blind, mask, mask_blind, mlwe, mask_mlwe (params.go:99-111)
    res_two_nm: float = None          # ResTwoNm() (params.go:432-435)
    in_com_dcmp_two_nm: float = None  # InComDcmpTwoNm() (params.go:437-440)

    @classmethod
    def from_dict(cls, P, field_q):
        return cls(rank=P["rank"], rows=P["rows"], cols=P["cols"], slots=P["slots"], exp=P["exp"], d=P["d"],
                   in_msis=P["in_msis"], out_msis=P["out_msis"], mlwe=P["mlwe"], dcmp=P["in_com_dcmp_len"],
                   log_in_cut=P["log_in_cut"], log_out_cut=P["log_out_cut"], base=P["base"], q=list(P["q"]),
                   qo=list(P["qo"]), field_q=int(field_q),
                   stddevs=tuple(P[k] for k in STDDEV_KEYS) if all(k in P for k in STDDEV_KEYS) else None,
                   res_two_nm=P.get("res_two_nm"), in_com_dcmp_two_nm=P.get("in_com_dcmp_two_nm"))

    @property
    def L(self):
        return (self.field_q.bit_length() + 63) // 64

    @property
    def nq(self):
        return len(self.q)

    @property
    def nqo(self):
        return len(self.qo)

    def c_struct(self):
        s = JindoParamsC()
        for k in ["rank", "rows", "cols", "slots", "exp", "d", "in_msis", "out_msis", "mlwe", "dcmp", "log_in_cut",
                  "log_out_cut"]:
            setattr(s, k, int(getattr(self, k)))
        s.base = self.base
        s.nq, s.nqo = self.nq, self.nqo
        for i, x in enumerate(self.q):
            s.q[i] = x
        for i, x in enumerate(self.qo):
            s.qo[i] = x
        s.field_limbs = self.L
        for i in range(self.L):
            s.field_q[i] = (self.field_q >> (64 * i)) & ((1 << 64) - 1)
        return s

    # array shapes (include/ringo.h rg_jindo_commit)
    def shapes(self, batch=None):
        nm = self.in_msis + self.mlwe
        sh = dict(last_row=(self.cols * self.slots, self.L), mask=(self.rows, self.slots, self.L),
                  enc_noise=(self.cols + 1, self.rows, self.d), mlwe_noise=(self.cols + 1, nm, self.d),
                  incom=(self.dcmp, self.nqo, self.d), enc=(self.cols + 1, self.rows, self.nq, self.d),
                  mlwe_out=(self.cols + 1, nm, self.nq, self.d), com=(self.out_msis, self.nq, self.d))
        if batch is not None:
            sh = {k: (batch,) + v for k, v in sh.items()}
        return sh

    def ck_shapes(self):
        return dict(ck_in=(self.in_msis, self.rows, self.nq, self.d),
                    ck_mlwe=(self.in_msis, self.mlwe, self.nq, self.d),
                    ck_out=(self.out_msis, self.dcmp, self.nqo, self.d))


@dataclass
class Randomness:
    """The draws Prover.Commit makes internally (prover.go:65-139), injected."""
    last_row: np.ndarray    # [cols*slots][L] Montgomery, last entry 0
    mask: np.ndarray        # [rows][slots][L]
    enc_noise: np.ndarray   # [cols+1][rows][d] int64
    mlwe_noise: np.ndarray  # [cols+1][inMSIS+mlwe][d] int64


@dataclass
class Opening:  # entities.go:103-107
    InCommit: np.ndarray
    Encode: np.ndarray
    MLWE: np.ndarray


@dataclass
class Commitment:  # entities.go:80-82
    Value: np.ndarray


def _words(shape):
    n = 1
    for x in shape:
        n *= int(x)
    return n


class Prover:
    def __init__(self, params, crs=None, ck=None, ck_dev=None, stream=None):
        """ck: host arrays (rg_jindo_create); ck_dev: device buffers on the current GPU, e.g. where
        an RCCL broadcast put the key (rg_jindo_create_dev: copied device-to-device); else the
        key is derived from `crs` (NewCommitKey, entities.go:21-73)."""
        self.params = params
        h = vp()
        ps = params.c_struct()
        if ck_dev is not None:
            sh = params.ck_shapes()
            a, b, c = (_addr(x, _words(sh[k])) for x, k in zip(ck_dev, ("ck_in", "ck_mlwe", "ck_out")))
            st = lib().rg_jindo_create_dev(ctypes.byref(ps), a, b, c, _stream(stream), ctypes.byref(h))
        elif ck is not None:
            a, b, c = (np.ascontiguousarray(x, np.uint64) for x in ck)
            st = lib().rg_jindo_create(ctypes.byref(ps), ptr(a), ptr(b), ptr(c), ctypes.byref(h))
        else:
            st = lib().rg_jindo_create_from_crs(ctypes.byref(ps), crs, len(crs), ctypes.byref(h))
        check(st)
        self.h = h
        self._L = lib()
        if params.stddevs is not None:
            sd = JindoStddevsC(*params.stddevs)
            check(lib().rg_jindo_set_stddevs(self.h, ctypes.byref(sd)))

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):  # the CDLL bound at creation
            self._L.rg_jindo_destroy(self.h)  # (module globals may already be gone at interpreter exit)
            self.h = None

    def commit_key(self):
        sh = self.params.ck_shapes()
        out = {k: np.zeros(v, np.uint64) for k, v in sh.items()}
        check(lib().rg_jindo_commit_key(self.h, ptr(out["ck_in"]), ptr(out["ck_mlwe"]), ptr(out["ck_out"])))
        return out["ck_in"], out["ck_mlwe"], out["ck_out"]

    def Commit(self, v, rnd):
        """Commit(v) (prover.go:45-62) with injected randomness; v: [n][L] Montgomery."""
        P = self.params
        v = np.ascontiguousarray(v, np.uint64)
        if v.shape[0] > P.rank:
            raise RingoPanic("len(v) > params.rank")
        sh = P.shapes()
        o = {k: np.zeros(sh[k], np.uint64) for k in ["incom", "enc", "mlwe_out", "com"]}
        args = [np.ascontiguousarray(rnd.last_row, np.uint64), np.ascontiguousarray(rnd.mask, np.uint64)]
        en = np.ascontiguousarray(rnd.enc_noise, np.int64)
        mn = np.ascontiguousarray(rnd.mlwe_noise, np.int64)
        check(lib().rg_jindo_commit(self.h, ptr(v), v.shape[0], ptr(args[0]), ptr(args[1]), iptr(en), iptr(mn),
                                    ptr(o["incom"]), ptr(o["enc"]), ptr(o["mlwe_out"]), ptr(o["com"])))
        return Commitment(o["com"]), Opening(o["incom"], o["enc"], o["mlwe_out"])

    def commit_key_dev(self):
        """Device addresses of the handle's commit key (ck_in, ck_mlwe, ck_out)."""
        a, b, c = vp(), vp(), vp()
        check(lib().rg_jindo_commit_key_dev(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def commit_dev(self, batch, v, nv, last_row, mask, enc_noise, mlwe_noise, incom, enc, mlwe, com, stream=None):
        """rg_jindo_commit_dev on device buffers (tensors or int addresses)."""
        sh = self.params.shapes(batch)
        w = {k: _words(x) for k, x in sh.items()}
        L = self.params.L
        check(lib().rg_jindo_commit_dev(self.h, batch, _addr(v, batch * nv * L), nv, _addr(last_row, w["last_row"]),
                                        _addr(mask, w["mask"]), _addr(enc_noise, w["enc_noise"]),
                                        _addr(mlwe_noise, w["mlwe_noise"]), _addr(incom, w["incom"]),
                                        _addr(enc, w["enc"]), _addr(mlwe, w["mlwe_out"]), _addr(com, w["com"]),
                                        _stream(stream)))

    def delta_inv(self):
        """Encoder.deltaInv (encoder.go:50-67) as the library computes it."""
        out = (ctypes.c_double * self.params.exp)()
        check(lib().rg_jindo_delta_inv(self.h, out))
        return list(out)

    def sample_dev(self, batch, v, nv, seeds, first_commit, last_row, mask, enc_noise, mlwe_noise, stream=None):
        """rg_jindo_sample_dev: the randomness Commit draws, on the device (layouts of commit_dev)."""
        sh = self.params.shapes(batch)
        sc = seeds.c_struct()
        check(lib().rg_jindo_sample_dev(self.h, batch, _addr(v, batch * nv * self.params.L), nv, ctypes.byref(sc),
                                        first_commit, _addr(last_row, _words(sh["last_row"])),
                                        _addr(mask, _words(sh["mask"])), _addr(enc_noise, _words(sh["enc_noise"])),
                                        _addr(mlwe_noise, _words(sh["mlwe_noise"])), _stream(stream)))

    def commit_sampled_dev(self, batch, v, nv, seeds, first_commit, incom, enc, mlwe, com, stream=None):
        """Prover.Commit end to end on the device: sampling + commit (rg_jindo_commit_sampled_dev)."""
        sh = self.params.shapes(batch)
        sc = seeds.c_struct()
        check(lib().rg_jindo_commit_sampled_dev(self.h, batch, _addr(v, batch * nv * self.params.L), nv,
                                                ctypes.byref(sc), first_commit, _addr(incom, _words(sh["incom"])),
                                                _addr(enc, _words(sh["enc"])), _addr(mlwe, _words(sh["mlwe_out"])),
                                                _addr(com, _words(sh["com"])), _stream(stream)))

    MAC_KINDS = {0: "generic", 1: "valu3", 2: "mfma"}  # include/ringo.h RG_MAC_*

    def mac_kinds(self):
        """(inner, outer): which kernel runs each Ajtai product of this handle."""
        a, b = ctypes.c_int(), ctypes.c_int()
        check(lib().rg_jindo_mac_kinds(self.h, ctypes.byref(a), ctypes.byref(b)))
        return self.MAC_KINDS[a.value], self.MAC_KINDS[b.value]

    def release_stream(self, stream=None):
        """Drop the scratch the handle caches for `stream` (rg_jindo_release_stream)."""
        check(lib().rg_jindo_release_stream(self.h, _stream(stream)))

    def commit_core(self, enc, mlwe):
        """The Ajtai core of Commit (prover.go:144-202) from NTT-domain Opening.Encode / MLWE:
        returns (Commitment.Value, Opening.InCommit)."""
        sh = self.params.shapes()
        enc = np.ascontiguousarray(enc, np.uint64)
        mlwe = np.ascontiguousarray(mlwe, np.uint64)
        if enc.shape != sh["enc"] or mlwe.shape != sh["mlwe_out"]:
            raise RingoPanic("inconsistent input(s)")
        incom, com = np.zeros(sh["incom"], np.uint64), np.zeros(sh["com"], np.uint64)
        check(lib().rg_jindo_commit_core(self.h, ptr(enc), ptr(mlwe), ptr(incom), ptr(com)))
        return com, incom

    def commit_core_dev(self, batch, enc, mlwe, incom, com, stream=None):
        sh = self.params.shapes(batch)
        check(lib().rg_jindo_commit_core_dev(self.h, batch, _addr(enc, _words(sh["enc"])),
                                             _addr(mlwe, _words(sh["mlwe_out"])), _addr(incom, _words(sh["incom"])),
                                             _addr(com, _words(sh["com"])), _stream(stream)))


    # ---- Prover.Evaluate (jindo/prover.go:205-324), device-resident, challenges injected ----
    # The Fiat-Shamir transcript stays with the caller (Go in the reference); these are Evaluate's
    # MulCoeffsMontgomeryThenAdd loops, and eval_point_dev / encode_challenges_dev (with
    # bigpoly.evaluate_batch_dev) build their inputs from the transcript's bytes on the device.
    def eval_shapes(self):
        P = self.params
        nm = P.in_msis + P.mlwe
        return dict(ob_incom=(P.dcmp, P.nqo, P.d), ob_enc=(P.cols + 1, P.rows, P.nq, P.d),
                    ob_mlwe=(P.cols + 1, nm, P.nq, P.d), partial=(P.cols + 1, P.nq, P.d),
                    pf_enc=(P.rows, P.nq, P.d), pf_mlwe=(nm, P.nq, P.d))

    def eval_batch_dev(self, batch, incom, enc, mlwe, bq, bo, ob_incom, ob_enc, ob_mlwe, stream=None):
        """openBatch = sum_i open[i] * batch[i] (prover.go:228-269); Proof.InCommit = ob_incom.
        bq = bo = None (params.batch == 1): openBatch = open[0]."""
        P, sh, es = self.params, self.params.shapes(batch), self.eval_shapes()
        w = lambda k: _words(sh[k])
        check(lib().rg_jindo_eval_batch_dev(self.h, batch, _addr(incom, w("incom")), _addr(enc, w("enc")),
                                            _addr(mlwe, w("mlwe_out")), _addr(bq, batch * P.nq * P.d),
                                            _addr(bo, batch * P.nqo * P.d), _addr(ob_incom, _words(es["ob_incom"])),
                                            _addr(ob_enc, _words(es["ob_enc"])), _addr(ob_mlwe, _words(es["ob_mlwe"])),
                                            _stream(stream)))

    def eval_reduce_dev(self, ob_incom, ob_enc, ob_mlwe, stream=None):
        """Words mod q in place (after summing partial openBatches across GPUs)."""
        es = self.eval_shapes()
        check(lib().rg_jindo_eval_reduce_dev(self.h, _addr(ob_incom, _words(es["ob_incom"])),
                                             _addr(ob_enc, _words(es["ob_enc"])), _addr(ob_mlwe, _words(es["ob_mlwe"])),
                                             _stream(stream)))

    def eval_partial_dev(self, ob_enc, left, partial, stream=None):
        """Proof.Partial[0..cols) and PartialMask (= partial[cols]) (prover.go:274-282)."""
        P, es = self.params, self.eval_shapes()
        check(lib().rg_jindo_eval_partial_dev(self.h, _addr(ob_enc, _words(es["ob_enc"])),
                                              _addr(left, P.rows * P.nq * P.d), _addr(partial, _words(es["partial"])),
                                              _stream(stream)))

    def eval_respond_dev(self, ob_enc, ob_mlwe, chals, pf_enc, pf_mlwe, stream=None):
        """Proof.Encode and Proof.MLWE (prover.go:300-314)."""
        P, es = self.params, self.eval_shapes()
        check(lib().rg_jindo_eval_respond_dev(self.h, _addr(ob_enc, _words(es["ob_enc"])),
                                              _addr(ob_mlwe, _words(es["ob_mlwe"])), _addr(chals, P.cols * P.nq * P.d),
                                              _addr(pf_enc, _words(es["pf_enc"])), _addr(pf_mlwe, _words(es["pf_mlwe"])),
                                              _stream(stream)))


    def eval_point_dev(self, x, left, right=None, stream=None):
        """left [rows][nq][d] = encode(leftVec(x)[j]) and, unless None, right [cols*slots][L] =
        rightVec(x) (utils.go:63-82) from the point x [L] on the device (rg_jindo_eval_point_dev)."""
        P = self.params
        check(lib().rg_jindo_eval_point_dev(self.h, _addr(x, P.L), _addr(left, P.rows * P.nq * P.d),
                                            _addr(right, P.cols * P.slots * P.L), _stream(stream)))

    def eval_point_multi_scratch_bytes(self, n_points):
        """Bytes of scratch eval_point_multi_dev needs (0 for an n_points outside [1, POINT_MAX_POINTS])."""
        return lib().rg_jindo_eval_point_multi_scratch_bytes(self.h, n_points)

    def eval_point_multi_dev(self, n_points, x, x_stride, left, right, scratch, stream=None):
        """eval_point_dev for n_points points in one asynchronous call (rg_jindo_eval_point_multi_dev):
        point k is the element at x + k * x_stride * L words, left [n_points][rows][nq][d], right
        [n_points][cols*slots][L] or None; scratch holds eval_point_multi_scratch_bytes(n_points) bytes."""
        P, n = self.params, n_points
        check(lib().rg_jindo_eval_point_multi_dev(
            self.h, n, _addr(x, ((n - 1) * x_stride + 1) * P.L if n else None), x_stride,
            _addr(left, n * P.rows * P.nq * P.d), _addr(right, n * P.cols * P.slots * P.L),
            _addr(scratch, self.eval_point_multi_scratch_bytes(n) // 8), _stream(stream)))

    def encode_challenges_dev(self, ring, bytes, n, out, stream=None):
        """encodeChallengeTo (utils.go:20-46) of n challenges: bytes, a device buffer of n * 16 bytes
        (a uint8 tensor or an int address), into out [n][nq or nqo][d] of ringQ (ring 0) or
        ringQOut (ring 1) (rg_jindo_encode_challenges_dev)."""
        P = self.params
        if ring not in (0, 1):
            raise RingoPanic("ring must be 0 (ringQ) or 1 (ringQOut)")
        check(lib().rg_jindo_encode_challenges_dev(self.h, ring, _byte_addr(bytes, 16 * n), n,
                                                   _addr(out, n * (P.nqo if ring else P.nq) * P.d), _stream(stream)))

    # ---- Evaluate for n_proofs proofs in two asynchronous calls around the transcript ----
    def eval_open_multi_scratch_bytes(self, n_proofs, batch):
        """Bytes of scratch eval_open_multi_dev needs (0 for arguments the call would refuse)."""
        return lib().rg_jindo_eval_open_multi_scratch_bytes(self.h, n_proofs, batch)

    def eval_open_multi_dev(self, n_proofs, batch, incom, enc, mlwe, open_proof_stride, open_commit_stride, x,
                            x_stride, batch_bytes, ob_enc, ob_mlwe, pf_incom, pf_partial, scratch, stream=None):
        """openBatch and Proof.InCommit / Partial / PartialMask of n_proofs proofs in one asynchronous call
        (rg_jindo_eval_open_multi_dev): opening t of proof p is open_proof_stride * p + open_commit_stride * t
        openings into incom / enc / mlwe, x and x_stride as eval_point_multi_dev, batch_bytes
        [n_proofs][batch][16] uint8; into ob_enc [n][cols+1][rows][nq][d], ob_mlwe [n][cols+1][nm][nq][d],
        pf_incom [n][dcmp][nqo][d], pf_partial [n][cols+1][nq][d].  batch_bytes = ob_enc = ob_mlwe = None iff
        batch == 1; scratch holds eval_open_multi_scratch_bytes(n_proofs, batch) bytes."""
        P, n, es = self.params, n_proofs, self.eval_shapes()
        last = ((n - 1) * open_proof_stride + (batch - 1) * open_commit_stride + 1) if n and batch else 0
        check(lib().rg_jindo_eval_open_multi_dev(
            self.h, n, batch, _addr(incom, last * _words(es["ob_incom"])), _addr(enc, last * _words(es["ob_enc"])),
            _addr(mlwe, last * _words(es["ob_mlwe"])), open_proof_stride, open_commit_stride,
            _addr(x, ((n - 1) * x_stride + 1) * P.L if n else None), x_stride, _byte_addr(batch_bytes, n * batch * 16),
            _addr(ob_enc, n * _words(es["ob_enc"])), _addr(ob_mlwe, n * _words(es["ob_mlwe"])),
            _addr(pf_incom, n * _words(es["ob_incom"])), _addr(pf_partial, n * _words(es["partial"])),
            _addr(scratch, self.eval_open_multi_scratch_bytes(n, batch) // 8), _stream(stream)))

    def eval_respond_multi_scratch_bytes(self, n_proofs):
        """Bytes of scratch eval_respond_multi_dev needs (0 for an n_proofs outside [1, EVAL_MAX_PROOFS])."""
        return lib().rg_jindo_eval_respond_multi_scratch_bytes(self.h, n_proofs)

    def eval_respond_multi_dev(self, n_proofs, ob_enc, ob_mlwe, ob_proof_stride, chal_bytes, pf_enc, pf_mlwe, scratch,
                               stream=None):
        """Proof.Encode and Proof.MLWE of n_proofs proofs in one asynchronous call
        (rg_jindo_eval_respond_multi_dev): the openBatch of proof p is ob_proof_stride * p openings into ob_enc /
        ob_mlwe (1 after eval_open_multi_dev; the openings and their proof stride when batch == 1), chal_bytes
        [n_proofs][cols][16] uint8; into pf_enc [n][rows][nq][d], pf_mlwe [n][nm][nq][d]; scratch holds
        eval_respond_multi_scratch_bytes(n_proofs) bytes."""
        P, n, es = self.params, n_proofs, self.eval_shapes()
        last = (n - 1) * ob_proof_stride + 1 if n else 0
        check(lib().rg_jindo_eval_respond_multi_dev(
            self.h, n, _addr(ob_enc, last * _words(es["ob_enc"])), _addr(ob_mlwe, last * _words(es["ob_mlwe"])),
            ob_proof_stride, _byte_addr(chal_bytes, n * P.cols * 16), _addr(pf_enc, n * _words(es["pf_enc"])),
            _addr(pf_mlwe, n * _words(es["pf_mlwe"])), _addr(scratch, self.eval_respond_multi_scratch_bytes(n) // 8),
            _stream(stream)))

    def evaluate_multi_transcript_dev(self, tr, com, incom, enc, mlwe, open_proof_stride, open_commit_stride, x,
                                      x_stride, batch_bytes, chal_bytes, ob_enc, ob_mlwe, pf_incom, pf_partial, pf_enc,
                                      pf_mlwe, open_scratch, respond_scratch, stream=None):
        """Prover.Evaluate (prover.go:220-316) of tr.n proofs with the transcript on the device, queued on
        `stream` with no host step in between: tr.open_dev (marshal x, absorb the crs, the commitments `com`
        and x, derive batch_bytes), eval_open_multi_dev, tr.respond_dev (absorb pf_partial, derive chal_bytes),
        eval_respond_multi_dev.  tr: a Transcript of this parameter set; batch_bytes [n][batch][16] and
        chal_bytes [n][cols][16] are uint8 device buffers the transcript writes; everything else as the
        two eval calls take it (batch_bytes = ob_enc = ob_mlwe = None iff batch == 1)."""
        n, batch = tr.n, tr.batch
        tr.open_dev(com, x, x_stride, batch_bytes, stream)
        self.eval_open_multi_dev(n, batch, incom, enc, mlwe, open_proof_stride, open_commit_stride, x, x_stride,
                                 batch_bytes, ob_enc, ob_mlwe, pf_incom, pf_partial, open_scratch, stream)
        tr.respond_dev(pf_partial, chal_bytes, stream)
        if batch == 1:
            self.eval_respond_multi_dev(n, enc, mlwe, open_proof_stride, chal_bytes, pf_enc, pf_mlwe, respond_scratch,
                                        stream)
        else:
            self.eval_respond_multi_dev(n, ob_enc, ob_mlwe, 1, chal_bytes, pf_enc, pf_mlwe, respond_scratch, stream)

    def challenge_bound(self):
        """Parameters.ChallengeBound() (params.go:357-360)."""
        b, ps = ctypes.c_uint64(), self.params.c_struct()
        check(lib().rg_jindo_challenge_bound(ctypes.byref(ps), ctypes.byref(b)))
        return b.value


def transcript_plans(params, crs, batch, poly_prefix, row_prefix, com_proof_stride=None, com_commit_stride=1):
    """The two absorb plans (xof.Plan) of the Jindo transcript (prover.go:220-302, verifier.go:56-96) for one
    parameter set, a state per proof:

      A  the crs (CommitKey.WriteRawTo), then each of the `batch` commitments' out_msis polynomials
         (Commitment.WriteRawTo), then x.Marshal().  Bases: 0 = the commitments, commitment t of proof p
         starting p * com_proof_stride + t * com_commit_stride commitments in (default (batch, 1): a
         [proof][commit][out_msis][nq][d] buffer; (1, n_proofs) reads the [commit][proof] buffer one
         commit_dev per round leaves behind); 1 = [n_proofs][8 * L] marshalled points (xof.marshal_dev).
      B  the cols + 1 polynomials of Partial / PartialMask.  Base 0 = pf_partial [n_proofs][cols+1][nq][d].

    The framing is the CALLER'S statement of Lattigo's ring.Poly.WriteTo, which is not in the reference
    tree and so is not pinned here: a polynomial of `levels` rows of n coefficients is written as
    poly_prefix(levels, n), then per row row_prefix(n) and the n coefficients as little-endian uint64,
    which is how the device holds a residue row.  Both callbacks return bytes (possibly empty).
    A plan holds at most 65,536 segments (one per row and one per distinct prefix run); xof.Plan raises
    for a set that needs more (batch 4096)."""
    from . import xof
    P = params
    row = P.d * 8
    pp, rp = bytes(poly_prefix(P.nq, P.d)), bytes(row_prefix(P.d))
    crs = bytes(crs)
    lit = crs + pp + rp
    o_pp, o_rp = len(crs), len(crs) + len(pp)

    def poly(segs, base, word_offset, stride):
        """one [nq][d] polynomial at `word_offset` words of base"""
        if pp or rp:
            segs.append((xof.LITERAL, o_pp, 0, len(pp) + len(rp)))  # the polynomial's prefix and its first row's: one run
        for l in range(P.nq):
            if l and rp:
                segs.append((xof.LITERAL, o_rp, 0, len(rp)))
            segs.append((base, (word_offset + l * P.d) * 8, stride, row))

    com_words = P.out_msis * P.nq * P.d
    ps = batch if com_proof_stride is None else com_proof_stride
    a = [(xof.LITERAL, 0, 0, len(crs))]
    for t in range(batch):
        for i in range(P.out_msis):
            poly(a, 0, t * com_commit_stride * com_words + i * P.nq * P.d, ps * com_words * 8)
    a.append((1, 0, 8 * P.L, 8 * P.L))
    b = []
    for i in range(P.cols + 1):
        poly(b, 0, i * P.nq * P.d, (P.cols + 1) * P.nq * row)
    return xof.Plan(a, lit), xof.Plan(b, lit)


class Transcript:
    """The Fiat-Shamir transcripts of n_proofs proofs of one parameter set on the device: the two plans of
    transcript_plans, the sponges (ringo.xof.Shake128) and the marshalled points.  open_dev and respond_dev
    only queue work on `stream`: nothing is copied to the host or waited for, so a batch Evaluate
    (Prover.evaluate_multi_transcript_dev) or Verify (Verifier.verify_multi_transcript_dev) is one
    uninterrupted queue.  Not safe for concurrent use, and one batch at a time: open_dev restarts it.

    Use it for large batches only.  Measured (profiles/xof_transcript_timing.txt, README "Transcript on the
    device"): the whole batched Evaluate with this transcript is faster than the host transcript between
    the two calls at 64 proofs (48.4 against 94.7 us per proof at t14_b1, 1,114 against 1,767 us at
    mult_t8193_b12) and slower at 1 and 8 proofs (a sponge is a serial chain, ~6 us per 168 bytes, whose
    time does not shrink with the batch): there keep the host flow (eval_open_multi_dev, hashlib / sha3,
    eval_respond_multi_dev)."""

    def __init__(self, params, crs, batch, n_proofs, poly_prefix, row_prefix, com_proof_stride=None,
                 com_commit_stride=1):
        import torch

        from . import xof
        from .bigpoly import Field
        self.params, self.batch, self.n = params, batch, n_proofs
        self.plan_a, self.plan_b = transcript_plans(params, crs, batch, poly_prefix, row_prefix, com_proof_stride,
                                                    com_commit_stride)
        self.field = Field(params.field_q, limbs=params.L)
        self.h = xof.Shake128(n_proofs)
        self.fork = xof.Shake128(n_proofs) if batch > 1 else None
        self.x_bytes = torch.empty(n_proofs * 8 * params.L, dtype=torch.uint8,
                                   device=torch.device("cuda", torch.cuda.current_device()))

    def open_dev(self, com, x, x_stride, batch_bytes, stream=None):
        """prover.go:220-248: x.Marshal(), absorb plan A; with batch > 1, fork (the copy replaces the
        reference's Reset-and-rewrite), squeeze batch * 16 bytes per proof from the fork into batch_bytes
        [n_proofs][batch][16] and absorb them into the original.  batch_bytes is None iff batch == 1."""
        from . import xof
        if (batch_bytes is None) != (self.batch == 1):
            raise RingoPanic("batch_bytes is None iff batch == 1")
        xof.marshal_dev(self.field, x, self.n, x_stride, self.x_bytes, stream=stream)
        self.h.reset(stream)
        self.h.absorb_plan(self.plan_a, [com, self.x_bytes], stream)
        if self.batch > 1:
            self.fork.copy_from(self.h, stream)
            self.fork.squeeze(batch_bytes, self.batch * 16, stream=stream)
            self.h.absorb(batch_bytes, self.batch * 16, stream=stream)

    def respond_dev(self, pf_partial, chal_bytes, stream=None):
        """prover.go:291-302: absorb Partial / PartialMask (plan B over pf_partial), squeeze cols * 16 bytes
        per proof into chal_bytes [n_proofs][cols][16]."""
        self.h.absorb_plan(self.plan_b, [pf_partial], stream)
        self.h.squeeze(chal_bytes, self.params.cols * 16, stream=stream)


def _byte_addr(x, nbytes):
    """Device address of a byte buffer: a contiguous uint8 tensor on the current GPU of at least
    nbytes, or a raw int address."""
    if x is None or isinstance(x, int):
        return x
    if str(x.dtype) != "torch.uint8":
        raise RingoPanic(f"byte buffer dtype {x.dtype}: need uint8")
    import torch
    if not x.is_contiguous() or x.device.type != "cuda" or x.device.index != torch.cuda.current_device():
        raise RingoPanic("byte buffer must be contiguous and on the current GPU")
    if x.numel() < nbytes:
        raise RingoPanic(f"byte buffer holds {x.numel()} bytes, need {nbytes}")
    return x.data_ptr()


class VerifyResultC(ctypes.Structure):  # include/ringo.h rg_jindo_verify_result
    _fields_ = [("outer_norm_sq", ctypes.c_uint64 * 10), ("inner_norm_sq", ctypes.c_uint64 * 10),
                ("outer_ok", ctypes.c_int), ("inner_ok", ctypes.c_int), ("consistency_ok", ctypes.c_int),
                ("eval_ok", ctypes.c_int), ("eval_lhs", ctypes.c_uint64 * 16), ("eval_rhs", ctypes.c_uint64 * 16),
                ("ok", ctypes.c_int)]


# include/ringo.h RG_JINDO_VERIFY_MAX_PROOFS, RG_JINDO_VERIFY_WORDS (tests/test_capi_jindo_verify_multi.py)
VERIFY_MAX_PROOFS = 65535
VERIFY_WORDS = 54
# include/ringo.h RG_JINDO_POINT_MAX_POINTS (tests/test_capi_jindo_verify_inputs.py)
POINT_MAX_POINTS = 65535
# include/ringo.h RG_JINDO_EVAL_MAX_PROOFS (tests/test_capi_jindo_eval_multi.py)
EVAL_MAX_PROOFS = 65535


@dataclass
class VerifyResult:
    ok: bool
    outer_ok: bool
    inner_ok: bool
    consistency_ok: bool
    eval_ok: bool
    outer_norm_sq: int
    inner_norm_sq: int
    eval_lhs: np.ndarray
    eval_rhs: np.ndarray


class Verifier:
    """NewVerifier (verifier.go:25-47): the commit key from the CRS and the rings' tables, on the
    device (the same deterministic state a Prover handle holds)."""

    def __init__(self, params, crs=None, ck=None):
        self.params = params
        self._p = Prover(params, crs=crs, ck=ck)
        self.h = self._p.h

    def eval_point_dev(self, x, left, right=None, stream=None):
        """encode(leftVec(x)) and rightVec(x) on the device (Prover.eval_point_dev)."""
        self._p.eval_point_dev(x, left, right, stream)

    def encode_challenges_dev(self, ring, bytes, n, out, stream=None):
        """encodeChallengeTo of n challenges on the device (Prover.encode_challenges_dev)."""
        self._p.encode_challenges_dev(ring, bytes, n, out, stream)

    def eval_point_multi_scratch_bytes(self, n_points):
        """Bytes of scratch eval_point_multi_dev needs (Prover.eval_point_multi_scratch_bytes)."""
        return self._p.eval_point_multi_scratch_bytes(n_points)

    def eval_point_multi_dev(self, n_points, x, x_stride, left, right, scratch, stream=None):
        """encode(leftVec(x)) and rightVec(x) of n_points points in one call (Prover.eval_point_multi_dev)."""
        self._p.eval_point_multi_dev(n_points, x, x_stride, left, right, scratch, stream)

    def verify_inputs_multi_scratch_bytes(self, n_proofs):
        """Bytes of scratch verify_inputs_multi_dev needs (0 for an n_proofs outside [1, POINT_MAX_POINTS])."""
        return lib().rg_jindo_verify_inputs_multi_scratch_bytes(self.h, n_proofs)

    def verify_inputs_multi_dev(self, n_proofs, batch, x, x_stride, batch_bytes, chal_bytes, bq, bo, chals, left,
                                right, scratch, stream=None):
        """Everything verify_multi_dev reads besides the proofs, from the transcripts' bytes, in one
        asynchronous call (rg_jindo_verify_inputs_multi_dev): x and x_stride as eval_point_multi_dev,
        batch_bytes [n_proofs][batch][16] and chal_bytes [n_proofs][cols][16] uint8 device buffers, into
        bq, bo, chals, left, right in verify_multi_dev's layouts; batch_bytes = bq = bo = None iff
        batch == 1; scratch holds verify_inputs_multi_scratch_bytes(n_proofs) bytes."""
        P, n, pq = self.params, n_proofs, self.params.nq * self.params.d
        check(lib().rg_jindo_verify_inputs_multi_dev(
            self.h, n, batch, _addr(x, ((n - 1) * x_stride + 1) * P.L if n else None), x_stride,
            _byte_addr(batch_bytes, n * batch * 16), _byte_addr(chal_bytes, n * P.cols * 16),
            _addr(bq, n * batch * pq), _addr(bo, n * batch * P.nqo * P.d), _addr(chals, n * P.cols * pq),
            _addr(left, n * P.rows * pq), _addr(right, n * P.cols * P.slots * P.L),
            _addr(scratch, self.verify_inputs_multi_scratch_bytes(n) // 8), _stream(stream)))

    def verify_dev(self, batch, com, bq, bo, chals, left, right, y, pf_incom, pf_partial, pf_enc, pf_mlwe,
                   stream=None):
        """Verify(x, com, y, pf) (verifier.go:50-133) on device buffers, challenges injected
        (include/ringo.h rg_jindo_verify_dev); bq = bo = None when params.batch == 1."""
        P = self.params
        if P.res_two_nm is None or P.in_com_dcmp_two_nm is None:
            raise RingoPanic("Parameters lack the two-norm bounds")
        r = VerifyResultC()
        nm, pq = P.in_msis + P.mlwe, P.nq * P.d
        check(lib().rg_jindo_verify_dev(self.h, batch, _addr(com, batch * P.out_msis * pq), _addr(bq, batch * pq),
                                        _addr(bo, batch * P.nqo * P.d), _addr(chals, P.cols * pq),
                                        _addr(left, P.rows * pq), _addr(right, P.cols * P.slots * P.L),
                                        _addr(y, batch * P.L), _addr(pf_incom, P.dcmp * P.nqo * P.d),
                                        _addr(pf_partial, (P.cols + 1) * pq), _addr(pf_enc, P.rows * pq),
                                        _addr(pf_mlwe, nm * pq), float(P.in_com_dcmp_two_nm), float(P.res_two_nm),
                                        ctypes.byref(r), _stream(stream)))
        return self._result(r)

    def _result(self, r):
        word = lambda w: sum(int(x) << (64 * i) for i, x in enumerate(w))
        L = self.params.L
        return VerifyResult(bool(r.ok), bool(r.outer_ok), bool(r.inner_ok), bool(r.consistency_ok), bool(r.eval_ok),
                            word(r.outer_norm_sq), word(r.inner_norm_sq), np.array(r.eval_lhs[:L], np.uint64),
                            np.array(r.eval_rhs[:L], np.uint64))

    def verify_multi_scratch_bytes(self, n_proofs, batch):
        """Bytes of scratch verify_multi_dev needs (0 for an n_proofs outside [1, VERIFY_MAX_PROOFS])."""
        return lib().rg_jindo_verify_multi_scratch_bytes(self.h, n_proofs, batch)

    def verify_multi_dev(self, n_proofs, batch, com, bq, bo, chals, left, right, y, pf_incom, pf_partial, pf_enc,
                         pf_mlwe, out, scratch, stream=None):
        """verify_dev for n_proofs proofs in one asynchronous call (rg_jindo_verify_multi_dev): every
        buffer has verify_dev's layout under a leading [n_proofs]; out [n_proofs][VERIFY_WORDS] receives
        the records (unpack_verify_words) once the stream has run; scratch holds
        verify_multi_scratch_bytes(n_proofs, batch) bytes."""
        P = self.params
        if P.res_two_nm is None or P.in_com_dcmp_two_nm is None:
            raise RingoPanic("Parameters lack the two-norm bounds")
        n, nm, pq = n_proofs, P.in_msis + P.mlwe, P.nq * P.d
        check(lib().rg_jindo_verify_multi_dev(
            self.h, n, batch, _addr(com, n * batch * P.out_msis * pq), _addr(bq, n * batch * pq),
            _addr(bo, n * batch * P.nqo * P.d), _addr(chals, n * P.cols * pq), _addr(left, n * P.rows * pq),
            _addr(right, n * P.cols * P.slots * P.L), _addr(y, n * batch * P.L), _addr(pf_incom, n * P.dcmp * P.nqo * P.d),
            _addr(pf_partial, n * (P.cols + 1) * pq), _addr(pf_enc, n * P.rows * pq), _addr(pf_mlwe, n * nm * pq),
            float(P.in_com_dcmp_two_nm), float(P.res_two_nm), _addr(out, n * VERIFY_WORDS),
            _addr(scratch, self.verify_multi_scratch_bytes(n, batch) // 8), _stream(stream)))

    def verify_multi_transcript_dev(self, tr, com, x, x_stride, y, pf_incom, pf_partial, pf_enc, pf_mlwe, batch_bytes,
                                    chal_bytes, bq, bo, chals, left, right, out, inputs_scratch, verify_scratch,
                                    stream=None):
        """Verifier.Verify (verifier.go:56-133) of tr.n proofs with the transcript replayed on the device,
        queued on `stream` with no host step in between: tr.open_dev and tr.respond_dev over the proofs'
        Partial (the bytes land in batch_bytes / chal_bytes), verify_inputs_multi_dev, verify_multi_dev.
        bq, bo, chals, left, right are the buffers verify_inputs_multi_dev fills; batch_bytes = bq = bo =
        None iff batch == 1; out [n][VERIFY_WORDS] as verify_multi_dev."""
        n, batch = tr.n, tr.batch
        tr.open_dev(com, x, x_stride, batch_bytes, stream)
        tr.respond_dev(pf_partial, chal_bytes, stream)
        self.verify_inputs_multi_dev(n, batch, x, x_stride, batch_bytes, chal_bytes, bq, bo, chals, left, right,
                                     inputs_scratch, stream)
        self.verify_multi_dev(n, batch, com, bq, bo, chals, left, right, y, pf_incom, pf_partial, pf_enc, pf_mlwe, out,
                              verify_scratch, stream)

    def unpack_verify_words(self, words):
        """The records of verify_multi_dev (host words [n][VERIFY_WORDS]) as verify_dev's result objects."""
        words = np.ascontiguousarray(words, np.uint64).reshape(-1, VERIFY_WORDS)
        out = []
        for rec in words:
            r = VerifyResultC()
            check(lib().rg_jindo_verify_unpack(rec.ctypes.data, self.params.L, ctypes.byref(r)))
            out.append(self._result(r))
        return out

    def VerifyMulti(self, batch, com, bq, bo, chals, left, right, y, pf_incom, pf_partial, pf_enc, pf_mlwe):
        """Host arrays in the verify_multi_dev layouts (the leading dimension is the proof): staged to
        the device, one verify_multi_dev, one synchronisation, the unpacked results."""
        import torch
        n = len(com)
        if n == 0:
            return []
        for a in (chals, left, right, y, pf_incom, pf_partial, pf_enc, pf_mlwe) + (() if bq is None else (bq, bo)):
            if len(a) != n:
                raise RingoPanic("the proofs' arrays differ in length")
        if any(len(c) != batch for c in com) or any(len(v) != batch for v in y):  # verifier.go:51-54
            raise RingoPanic("len(v) != params.batch")
        dev = torch.device("cuda", torch.cuda.current_device())
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
        args = [t(a) for a in (com, bq, bo, chals, left, right, y, pf_incom, pf_partial, pf_enc, pf_mlwe)]
        out = torch.empty((n, VERIFY_WORDS), dtype=torch.int64, device=dev)
        scratch = torch.empty(self.verify_multi_scratch_bytes(n, batch) // 8, dtype=torch.int64, device=dev)
        self.verify_multi_dev(n, batch, *args, out, scratch)
        return self.unpack_verify_words(out.cpu().numpy().view(np.uint64))

    def Verify(self, batch, com, bq, bo, chals, left, right, y, pf_incom, pf_partial, pf_enc, pf_mlwe):
        """Host arrays (numpy) in the verify_dev layouts: staged to the device, then verify_dev."""
        import torch
        if len(com) != batch or len(y) != batch:  # verifier.go:51-54
            raise RingoPanic("len(v) != params.batch")
        dev = torch.device("cuda", torch.cuda.current_device())
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)
        args = [t(a) for a in (com, bq, bo, chals, left, right, y, pf_incom, pf_partial, pf_enc, pf_mlwe)]
        return self.verify_dev(batch, *args)


def NewVerifier(params, crs):
    return Verifier(params, crs=crs)


def uniform_words_dev(seed, instance, first_word, n, out, stream=None):
    """UniformSampler.Sample() words [first_word, first_word + n) of instance `instance` of
    NewUniformSamplerWithSeed(seed) into the device buffer `out` (rg_uniform_words_dev)."""
    check(lib().rg_uniform_words_dev(bytes(seed), len(seed), instance, first_word, n, _addr(out, n), _stream(stream)))


def NewProver(params, crs):
    return Prover(params, crs=crs)
