"""Test-side model of PAIRED bootstrapping (include/fhelin.h "Paired bootstrapping"), residue for residue.

Not part of the oracle: a composition over oracle.residue_boot.ResidueBootstrapper that states pair(a, b, drop) from that class's own
pieces - rev.level_reduce / mult_int / rescale / add / sub, then mult_i, apply, conjugate, eval_mod and the ModRaise / SubSum body of
mod_raise - in the order the definition gives.  It adds no arithmetic of its own: every residue comes out of an oracle function."""
import numpy as np

import oracle as orc
from oracle.residue_boot import ResidueBootstrapper
from oracle.residue_eval import LD, RCt, _llround


class PairBootstrapper(ResidueBootstrapper):
    def _scaled(self, ct):
        """step 1 for one input: (y_x = k0_x x on two limbs at scale x.scale k0_x, rho_x as mod_raise computes it for x alone)"""
        rev = self.rev
        corr = self.desc["correction"]
        x = rev.rescale(ct) if ct.deg >= 2 else ct
        assert x.npoly == 2 and x.ell >= 2
        x = rev.level_reduce(x, 2)
        q0, q1 = LD(int(rev.q[0])), LD(int(rev.q[1]))
        target = q0 / LD(1 << corr)
        k0 = _llround(target * q1 / x.scale)
        assert k0 >= 2
        y = rev.mult_int(x, k0, True, x.scale * LD(k0))
        rho = rev.rescale(y).scale * LD(1 << corr) / q0
        return y, rho

    def _raise(self, x, top_ell):
        """ModRaise of the one-limb x to top_ell limbs and SubSum: the body of ResidueBootstrapper.mod_raise"""
        rev = self.rev
        up = RCt(orc.modraise(x.d[:, 0], top_ell, rev.q[:top_ell], rev.psi_q[:top_ell]), 1, rev.sf[0])
        gap = (self.N // 2) // self.n
        j = 1
        while j < gap:
            idx = self.n * j
            r = orc.rotate(up.d, rev.keys[idx], orc.galois(rev.log_n, idx), rev.alpha, rev.q, rev.p, rev.psi_q, rev.psi_p)
            up = rev.add(up, RCt(r, up.deg, up.scale))
            j <<= 1
        return up

    def pair(self, a, b, stop_after=0, drop=0):
        """(A, Bv), or the pipeline's one ciphertext after stage stop_after in 1..3"""
        rev, n = self.rev, self.n
        packed = self.desc["packed"]
        corr = self.desc["correction"]
        assert corr >= 1
        ya, rho_a = self._scaled(a)
        yb, rho_b = self._scaled(b)
        p = rev.add(ya, self.mult_i(yb))                       # two limbs, y_a's scale
        p = rev.rescale(p)
        w = self._raise(p, len(rev.q) - drop)
        if stop_after == 1:
            return w
        for st in self.desc["c2s"]:
            w = self.apply(st, w, n)
        ns = 2 * n if packed else n
        wc = self.conjugate(w)
        re = rev.add(w, wc)
        if stop_after == 2:
            return re
        if packed:
            v = self.eval_mod(re)
            if stop_after == 3:
                return v
        else:
            im = self.mult_i(rev.sub(wc, w))
            if stop_after == 3:
                return self.eval_mod(re)
            va, vb = self.eval_mod(re), self.eval_mod(im)
            v = rev.add(va, self.mult_i(vb))
        for i, st in enumerate(self.desc["s2c"]):
            v = self.apply(st, v, ns)
            if packed and i == 0:
                ns = n
        v = rev.mult_int(v, 1 << (corr - 1), False, v.scale)   # half of the single bootstrap's 2^corr: the slots hold (a + i b) / 2
        if v.deg >= 2:
            v = rev.rescale(v)
        vc = self.conjugate(v)
        A = rev.add(v, vc)
        Bv = self.mult_i(rev.sub(vc, v))
        A.scale = v.scale * rho_a
        Bv.scale = v.scale * rho_b
        return A, Bv
