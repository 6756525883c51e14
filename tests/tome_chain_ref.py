"""The materialised VidToMe chain, kept as the reference of tests/test_gpu_kernels.py::test_vidtome_chain_equals_materialised_reference.

This is the chain `VidToMe.compute_merge` ran before it carried the cosine-normalised rows beside the tokens, moved here unchanged in substance: every
round GATHERs its survivors into a buffer of their own, the global stage copies local tokens and bank together (`cat`), and every match NORMALISES the
sequence it is given (norm1's metric serves the first round only).  Normalisation is per row, so `normalise(gather(x)) == gather(normalise(x))` bit for
bit, and every map, merged row and bank of this chain must equal what tc_light_amd/vidtome.py computes -- with `torch.equal`, no tolerance.

Built from leaf C-ABI calls alone.  Of tc_light_amd/vidtome.py it uses `VidToMe._positions` and `VidToMe.round_frames` (index tables) and nothing else:
it owns its bank dict, and takes each chunk's (F, randfs, coin) explicitly instead of drawing them.
"""
import torch

from tc_light_amd.lib import lib, stream
from tc_light_amd.vidtome import VidToMe

H16 = torch.float16
I32 = torch.int32


class ChainRef:
    def __init__(self, device="cuda", local_merge_ratio=0.6, merge_global=True, global_merge_ratio=0.5, align_batch=True, target_stride=4, global_rand=0.5):
        self.dev = torch.device(device)
        self.args = dict(local_merge_ratio=local_merge_ratio, merge_global=merge_global, global_merge_ratio=global_merge_ratio, align_batch=align_batch,
                         target_stride=target_stride, global_rand=global_rand)
        self.tables = VidToMe(device, align_batch=align_batch, target_stride=target_stride)      # _positions / round_frames only
        self.banks = {}                 # block name -> contiguous [ne, Tb, C] f16
        self.trace = []
        self._ws = None
        self.L = lib()

    def _range(self, lo, hi):
        return torch.arange(lo, hi, dtype=I32, device=self.dev)

    def _gather(self, s1, bs1, mp, out, bso, n, C, nb=2):
        L = self.L
        if mp is None or mp.dim() == 1:
            L.tcl_gather_rows_f16(s1, bs1, 0, 0, mp if mp is not None else 0, out, bso, nb, n, C, stream())
        else:
            f1, fo = s1.reshape(-1), out.reshape(-1)
            for b in range(nb):
                L.tcl_gather_rows_f16(f1[b * bs1:], bs1, 0, 0, mp[b], fo[b * bso:], bso, 1, n, C, stream())

    def _compose(self, outer, inner, off, n):
        """out[i] = outer[off + inner[i]] (inner None = identity), per batch entry when either map is."""
        L = self.L
        per = outer.dim() == 2 or (inner is not None and inner.dim() == 2)
        if not per:
            out = torch.empty(n, dtype=I32, device=self.dev)
            L.tcl_index_compose(outer, inner if inner is not None else 0, off, n, out, stream())
            return out
        nb = outer.shape[0] if outer.dim() == 2 else inner.shape[0]
        out = torch.empty(nb, n, dtype=I32, device=self.dev)
        for b in range(nb):
            L.tcl_index_compose(outer[b] if outer.dim() == 2 else outer, (inner[b] if inner.dim() == 2 else inner) if inner is not None else 0,
                                off, n, out[b], stream())
        return out

    def _match(self, tokens, T, C, a_pos, na, b_pos, nb, ratio, tbs=None, affine=None, metric=None, ne=2):
        """tokens: ne [T, C] slices tbs elements apart (default T*C: a contiguous [ne, T, C]) -> (mrg [na-r+nb], unm [T]) int32 maps ([ne, .] each
        without align_batch).  metric: the tokens' cosine-normalised rows in the same layout when the caller has them; otherwise normalised here."""
        L = self.L
        r = min(na, int(na * ratio))                                            # merge.py:90
        mbs = T * C                                                             # elements between the two batch entries of the metric
        if metric is not None:
            metric, mbs = metric.reshape(-1), (T * C if tbs is None else tbs)
        else:
            metric = torch.empty(ne * T * C, dtype=H16, device=self.dev)
            if ne == 1 or tbs is None or tbs == T * C:
                L.tcl_tome_normalize_f16(tokens, metric, ne * T, C, stream())
            else:
                flat = tokens.reshape(-1)
                L.tcl_tome_normalize_f16(flat, metric, T, C, stream())
                L.tcl_tome_normalize_f16(flat[tbs:], metric[T * C:], T, C, stream())
        need = L.tcl_tome_match_workspace_bytes(na)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.zeros(need, dtype=torch.uint8, device=self.dev)        # zeroed once; every match leaves it zero again
        aligned = self.args["align_batch"]
        shape = (na - r + nb,) if aligned else (ne, na - r + nb)
        mrg = torch.empty(shape, dtype=I32, device=self.dev)
        unm = torch.empty((T,) if aligned else (ne, T), dtype=I32, device=self.dev)
        for b in range(1 if aligned else ne):                                   # aligned: ONE matching over both entries (scores concatenated along dst)
            mt, mo, uo, Bt = (metric, mrg, unm, ne) if aligned else (metric[b * mbs:], mrg[b], unm[b], 1)
            if affine is not None:
                L.tcl_tome_match_affine_f16(mt, mbs, Bt, C, a_pos, na, b_pos, nb, r, affine[0], affine[1], affine[2], mo, uo, self._ws, stream())
            else:
                L.tcl_tome_match_f16(mt, mbs, Bt, C, a_pos, na, b_pos, nb, r, mo, uo, self._ws, stream())
        return mrg, unm, na - r + nb

    def compute_merge(self, name, x, F, randfs, coin, N, C, xbs=None, metric=None, ne=2):
        """One chunk of F frames with the draws (randfs: one per randframe round, coin) -> (merged rows [ne, T, C], unm or None, T); appends the
        trace dict VidToMe.trace records."""
        a, L = self.args, self.L
        if xbs is None:
            xbs = F * N * C
        # ---- local merging (patch.py:36-58): randframe rounds until one frame is left
        mrg1 = unm1 = None
        seq, sbs, T, unm_pre = x, xbs, F * N, 0
        for cur, randf in zip(*self.tables.round_frames(F, randfs)):
            a_pos, b_pos = self.tables._positions(cur, N, randf, unm_pre)
            single = unm_pre == 0 and cur <= a["target_stride"]                # dst = the N tokens of frame randf, src = the rest: affine
            mrg, unm, Tn = self._match(seq, T, C, a_pos, a_pos.numel(), b_pos, b_pos.numel(), a["local_merge_ratio"], tbs=sbs,
                                       affine=(randf * N, N, randf * N) if single else None, metric=metric if seq is x else None, ne=ne)
            nxt = torch.empty(ne, Tn, C, dtype=H16, device=self.dev)
            self._gather(seq, sbs, mrg, nxt, Tn * C, Tn, C, ne)
            if mrg1 is None:
                mrg1, unm1 = mrg, unm
            else:
                mrg1 = self._compose(mrg1, mrg, 0, Tn)                          # merged slot -> row of the joined input
                unm1 = self._compose(unm, unm1, 0, F * N)                       # joined position -> slot of the current sequence
            unm_pre += Tn - b_pos.numel()                                       # ret_dict["unm_num"] = na - r
            seq, sbs, T = nxt, Tn * C, Tn
        if F > 1:
            local, TL = seq, T
        else:
            TL = N                                       # F == 1: nothing to merge locally; keep the [ne, T, C] layout
            if xbs == N * C or ne == 1:
                local = x.reshape(-1)[:ne * N * C].view(ne, N, C)
            else:
                local = torch.empty(2, N, C, dtype=H16, device=self.dev)
                L.tcl_gather_rows_f16(x, xbs, 0, 0, 0, local, N * C, 2, N, C, stream())
        if not a["merge_global"]:
            return local, unm1, TL
        bank = self.banks.get(name)
        if bank is None:                                                        # patch.py:81-82: the first chunk seeds the bank
            self.banks[name] = local if F > 1 else local.clone()
            self.trace.append(dict(name=name, F=F, unm=unm1, gather=mrg1, mrg1=mrg1, T=TL))
            return local, unm1, TL
        assert bank.shape[0] == ne
        Tb = bank.shape[1]
        src_len, loff, boff = (TL, 0, TL) if coin > a["global_rand"] else (Tb, Tb, 0)      # local tokens are src on a coin above global_rand (patch.py:61-70)
        T = TL + Tb
        cat = torch.empty(ne, T, C, dtype=H16, device=self.dev)
        L.tcl_gather_rows_f16(local, TL * C, 0, 0, 0, cat[:, loff:], T * C, ne, TL, C, stream())
        L.tcl_gather_rows_f16(bank, bank.stride(0), 0, 0, 0, cat[:, boff:], T * C, ne, Tb, C, stream())
        mrg2, unm2, Tm = self._match(cat, T, C, self._range(0, src_len), src_len, self._range(src_len, T), T - src_len,
                                     a["global_merge_ratio"], affine=(src_len, 0, src_len), ne=ne)
        merged = torch.empty(ne, Tm, C, dtype=H16, device=self.dev)
        self._gather(cat, T * C, mrg2, merged, Tm * C, Tm, C, ne)
        unm = self._compose(unm2, unm1, loff, F * N)                            # 2s-unmerge then the randframe unmerges (func_warper(u_ls[::-1]))
        bmap = self._compose(mrg2, unm2[..., loff:].contiguous() if unm2.dim() == 2 else unm2[loff:], 0, TL)     # bank <- u(merged_tokens) (patch.py:80)
        nb_ = torch.empty(ne, TL, C, dtype=H16, device=self.dev)
        self._gather(cat, T * C, bmap, nb_, TL * C, TL, C, ne)
        self.banks[name] = nb_
        self.trace.append(dict(name=name, F=F, unm=unm, mrg2=mrg2, mrg1=mrg1, T=Tm, loff=loff, boff=boff, TL=TL, bmap=bmap))
        return merged, unm, Tm
