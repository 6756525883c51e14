"""VidToMe token merging, host side (device-resident state, HIP kernels for all arithmetic).

Mirrors utils/VidToMe/vidtome/patch.py: `apply_patch(...)` arguments live in `VidToMe.args`, `update_patch(pipe,
global_tokens=None)` is `VidToMe.reset_global_tokens()`, and `compute_merge` (patch.py:14-91) runs per patched
transformer block.  Differences, all deliberate and documented in DESIGN.md:
  * the global-token bank of each block stays in HBM (the reference copies it to the CPU and back, patch.py:65-82);
  * the random choices (`randf`, merge.py:56-58; the src/dst coin, patch.py:61) come from an explicit host stream of
    draws shared by all blocks of one UNet forward -- in the reference every block owns a generator forked from the same
    state, so they draw identical numbers in lock-step (vidtome/utils.py:18-30, patch.py:215-231);
  * ties in the greedy matching are broken deterministically (csrc/merge.hip header).

`compute_merge` is ONE chain.  The cosine-normalised rows (the matching metric) are CARRIED beside the tokens instead of re-derived: normalisation is per
row, so `normalise(gather(x)) == gather(normalise(x))` bit for bit, and wherever tokens move through a map their metric moves through the same map in
the same launch (tcl_gather_rows_pair_f16).  Nothing is copied together either: the survivors of the last local round are gathered straight into their
slot of the [local | bank] block, and a bank is written straight into its slot of the block of the chunk that will meet it.  The chain that materialises
every stage (gather -> `cat` copy -> normalise -> match) lives on as the test reference, tests/tome_chain_ref.py: same maps, tokens and banks, bit for bit.
"""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from .lib import lib, stream

H16 = torch.float16
I32 = torch.int32


class Merged(NamedTuple):
    """The merged token sequence of one chunk, as compute_merge hands it to attn1: entry b's row t is row `index[t]` (row t when index is None) of
    `block[b]`.  Materialised sequences are Merged(contiguous [ne, T, C], T*C, None); a lazily merged one leaves the gather by `index` to the
    consumer's operand load (tcl_gemm_qkv_panels_f16)."""
    block: torch.Tensor                 # [ne, Tcat, C] f16, possibly a strided view (a bank in its slot of the next chunk's [src | dst] block)
    entry_stride: int                   # elements between batch entries
    index: Optional[torch.Tensor]       # int32 [T] shared by the entries, or None: the rows are already in place


class VidToMe:
    def __init__(self, device, local_merge_ratio=0.6, merge_global=True, global_merge_ratio=0.5, max_downsample=2, seed=123,
                 batch_size=2, align_batch=True, target_stride=4, global_rand=0.5, enabled=True):
        if batch_size != 2:
            raise NotImplementedError("TC-Light runs VidToMe with batch_size=2 (uncond, cond)")
        self.dev = torch.device(device)
        self.args = dict(local_merge_ratio=local_merge_ratio, merge_global=merge_global, global_merge_ratio=global_merge_ratio,
                         max_downsample=max_downsample, seed=seed, batch_size=batch_size, align_batch=align_batch,
                         target_stride=target_stride, global_rand=global_rand)
        self.enabled = enabled
        self.rng = np.random.default_rng(seed)
        self.banks = {}                 # block name -> [2, Tb, C] f16 (module.global_tokens, patch.py:60-82); may be a strided view (see _home)
        self._bank_met = {}             # block name -> the bank's cosine-normalised rows, same shape / strides
        self._home = {}                 # block name -> the [src | dst] blocks of the NEXT chunk, which already hold this bank in their slot (compute_merge)
        self._cur = (None, 0)
        self._pos = {}
        self._ws = None
        self.draws = None               # optional injected (randf, coin) for the next forwards (parity tests); randf: int or one per round
        self.trace = None               # set to a list to record per-block maps (parity tests)
        self.L = lib()

    # ---- reference surface
    def reset_global_tokens(self):      # vidtome.update_patch(pipe, global_tokens=None)  (generate_utils.py:235-238)
        self.banks.clear()
        self._bank_met.clear()
        self._home.clear()

    def begin_forward(self, F, size):
        """One UNet forward over one chunk: fix the draws every patched block will see (lock-step generators of the reference)."""
        self.begin_step([F], size)
        self.select_chunk(0)

    def round_frames(self, F, randfs=None):
        """Frame counts of the randframe rounds of an F-frame chunk (patch.py:43-56): the dst set of a round is every frame f with
        f % min(target_stride, frames) == randf, and those frames are what the next round sees -- 4 -> [4], 8 -> [8, 2], 16 -> [16, 4].
        Draws one randf per round (or checks the given ones) -> (frame counts, randfs)."""
        counts, out, cur, k = [], [], F, 0
        while cur > 1:
            ts = min(self.args["target_stride"], cur)
            rf = int(randfs[k]) if randfs is not None else int(self.rng.integers(0, ts))
            counts.append(cur); out.append(rf)
            cur = sum(1 for f in range(cur) if f % ts == rf)
            k += 1
        return counts, out

    def begin_step(self, Fs, size):
        """One UNet pass over the chunks Fs (reference chunk order): draw each chunk's (randf per round, coin) in that order."""
        self.size = size
        self._chunks = []
        for F in Fs:
            if self.draws is not None:
                randf, coin = self.draws.pop(0)
                randfs = self.round_frames(F, list(randf) if isinstance(randf, (list, tuple)) else [randf])[1]
            else:
                randfs = self.round_frames(F)[1]
                coin = float(self.rng.random())
            self._chunks.append((F, randfs, coin))

    def select_chunk(self, i):
        """Make chunk i of the last begin_step the current one."""
        self._cur = (self._chunks, i)
        self.F, self.randfs, self.coin = self._chunks[i]
        self.randf = self.randfs[0] if self.randfs else -1

    # ---- helpers
    def _positions(self, F, N, randf, unm_pre=0):
        """merge.py:44-67: the sequence is [unm_pre | F frames of N tokens]; src = the tokens of the frames f with f % min(stride, F) != randf,
        dst = the other frames' tokens followed by the unm_pre leading tokens."""
        key = (F, N, randf, unm_pre)
        hit = self._pos.get(key)
        if hit is None:
            idx = torch.arange(F * N, dtype=I32)
            dst = (idx // N) % min(self.args["target_stride"], F) == randf
            b = torch.cat([idx[dst] + unm_pre, torch.arange(unm_pre, dtype=I32)])
            hit = self._pos[key] = ((idx[~dst] + unm_pre).contiguous().to(self.dev), b.contiguous().to(self.dev))
        return hit

    def _range(self, lo, hi):
        key = ("r", lo, hi)
        hit = self._pos.get(key)
        if hit is None:
            hit = self._pos[key] = torch.arange(lo, hi, dtype=I32, device=self.dev)
        return hit

    # Maps are int32 tensors: 1-D when the two batch entries share the matching (align_batch, merge.py:93-108), [2, n] when every entry has
    # its own (merge.py:109-118).  The helpers below hide the difference from compute_merge.
    def _each(self, mp, nb, launch, *blocks):
        """launch(map, entries, *tensors) once over all nb batch entries when they share `mp` (1-D, or None = identity), else once per entry b with
        mp[b] and every block from its entry b on.  blocks: (tensor or None, elements between its batch entries)."""
        if mp is None or mp.dim() == 1:
            launch(mp, nb, *(t for t, _ in blocks))
        else:
            for b in range(nb):
                launch(mp[b], 1, *(None if t is None else torch.as_strided(t, (1,), (1,), t.storage_offset() + b * bs) for t, bs in blocks))

    def _gather(self, s1, bs1, mp, out, bso, n, C, nb=2):
        self._each(mp, nb, lambda m, e, s, o: self.L.tcl_gather_rows_f16(s, bs1, 0, 0, m, o, bso, e, n, C, stream()), (s1, bs1), (out, bso))

    def _move(self, sa, bsa, sb, bsb, mp, oa, boa, ob, bob, n, C, nb):
        """oa[b][i] = sa[b][mp[i]] and ob[b][i] = sb[b][mp[i]] in one launch: a token block and its metric through the same map (sb = ob = None: tokens only)."""
        self._each(mp, nb, lambda m, e, a, b, c, d: self.L.tcl_gather_rows_pair_f16(a, bsa, b, bsb, m, c, boa, d, bob, e, n, C, stream()),
                   (sa, bsa), (sb, bsb), (oa, boa), (ob, bob))

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

    def _merged(self, cat, T, mrg, Tm, C, ne, lazy):
        if lazy and mrg.dim() == 1:
            return Merged(cat, T * C, mrg)
        out = torch.empty(ne, Tm, C, dtype=H16, device=self.dev)
        self._gather(cat, T * C, mrg, out, Tm * C, Tm, C, ne)
        return Merged(out, Tm * C, None)

    def unmerge_add(self, h, bsh, y, T, unm, n, C, nb=2):
        """h[b][i] += y[b][unm[i]]: unmerge of attn1's output + residual (patch.py:178-179); unm None = identity."""
        self._each(unm, nb, lambda m, e, hh, yy: self.L.tcl_gather_add_rows_f16(hh, bsh, yy, T * C, m, e, n, C, stream()), (h, bsh), (y, T * C))

    def _match(self, metric, mbs, T, C, a_pos, na, b_pos, nb, ratio, affine=None, ne=2):
        """metric: the cosine-normalised rows of ne [T, C] token slices, mbs elements apart -> (mrg [na-r+nb], unm [T], na-r+nb) int32 maps ([ne, .]
        each without align_batch).  ne: batch entries present (1: the unconditional / conditional pair is known to be identical, see compute_merge).
        affine = (a_split, a_gap, b0): a_pos[i] = i if i < a_split else i + a_gap, b_pos[j] = b0 + j (true of the single-round VidToMe matches;
        lets the C = 320 matches take the strip-resident kernel, csrc/merge.hip::k_tome_match320 -- same maps, bit for bit)."""
        L = self.L
        r = min(na, int(na * ratio))                                            # merge.py:90
        metric = metric.reshape(-1)
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

    def _local_len(self, F, N):
        """Tokens a single-round chunk of F frames keeps after the local merge (merge.py:90: r = min(na, int(na * ratio)))."""
        if F <= 1:
            return N
        na = (F - 1) * N
        return na - min(na, int(na * self.args["local_merge_ratio"])) + N

    def _slots(self, coin, TL, Tb):
        """(src_len, loff, boff) of the global match's [src | dst] block: local tokens are src on a coin above global_rand, else the bank's (patch.py:61-70)."""
        return (TL, 0, TL) if coin > self.args["global_rand"] else (Tb, Tb, 0)

    def _next_block(self, ne, TL_bank, N, C):
        """If the chunk that will meet the bank this chunk leaves is known (the next one of the pass) and has one local round, allocate ITS [src | dst]
        token and metric blocks now and return where the bank goes in them: (cat, catm, TL_next, loff, boff).  The bank is then written once, into place."""
        lst, i = self._cur
        if lst is None or i + 1 >= len(lst):
            return None
        Fn, _, coin_n = lst[i + 1]
        if Fn > self.args["target_stride"]:
            return None
        TLn = self._local_len(Fn, N)
        _, loff, boff = self._slots(coin_n, TLn, TL_bank)
        T = TLn + TL_bank
        return (torch.empty(ne, T, C, dtype=H16, device=self.dev), torch.empty(ne, T, C, dtype=H16, device=self.dev), TLn, loff, boff)

    def _bank_slot(self, name, ne, TL, N, C):
        """Where the bank this chunk leaves goes -> (tok, met) [ne, TL, C]: its slot of the next chunk's blocks (`_next_block`, kept in _home) or new buffers."""
        nxt = self._next_block(ne, TL, N, C)
        if nxt is None:
            return torch.empty(ne, TL, C, dtype=H16, device=self.dev), torch.empty(ne, TL, C, dtype=H16, device=self.dev)
        cat_n, catm_n, _, _, boff_n = self._home[name] = nxt
        return cat_n[:, boff_n:boff_n + TL], catm_n[:, boff_n:boff_n + TL]

    # ---- patch.py:14-91
    def merges(self, N):
        """patch.py:15-18: does a block with N tokens per frame merge at all?"""
        if not self.enabled:
            return False
        return int(math.ceil(math.sqrt((self.size[0] * self.size[1]) // N))) <= self.args["max_downsample"]

    def compute_merge(self, name, x, F, N, C, xbs=None, metric=None, ne=2, lazy_merged=False):
        """x: norm1 output of one chunk: the unconditional [F*N, C] rows at x, the conditional ones xbs elements further (default
        F*N*C: a contiguous [2F, N, C] == joined [2, F*N, C]); metric: x's cosine-normalised rows in the same layout if norm1 wrote them
        (unet.py: tcl_layernorm_metric_f16), else None.  ne = 1: x holds ONE entry because the caller knows the pair to be identical (the
        classifier-free-guidance pair before the first text cross-attention, unet.py): with equal scores in both entries the matching picks
        the first one (lowest concatenated dst index), i.e. exactly the single-entry matching -- same maps, merged tokens and bank [1, T, C].
        Returns None when this block is not merged, else
        (Merged, unm int32 [F*N] ([2, F*N] without align_batch) or None for identity, T).
        lazy_merged=True: a merged sequence that is a gather of the [local | bank] block by a map shared by the entries is NOT materialised (see Merged)."""
        a = self.args
        if not self.merges(N):
            return None
        FN = F * N
        if xbs is None:
            xbs = FN * C
        seq, sbs, met, mbs = x, xbs, metric, xbs                               # the current sequence and its metric: ne slices sbs / mbs elements apart
        if met is None and (F > 1 or a["merge_global"]):                        # norm1 did not write it (direct callers / TCL_LN_METRIC=0)
            met, mbs = torch.empty(ne, FN, C, dtype=H16, device=self.dev), FN * C
            flat = x.reshape(-1)
            for b in range(ne):
                self.L.tcl_tome_normalize_f16(flat[b * xbs:], met[b], FN, C, stream())
        # ---- local merging (patch.py:36-58): randframe rounds until one frame is left -- one round for F <= target_stride (every TC-Light
        # config), 8 -> 2 -> 1 / 16 -> 4 -> 1 for longer chunks, the unmerged tokens of a round riding along as extra dst tokens of the next.
        # After the loop the local tokens are the rows `mrg` (None: all) of seq, TL of them; mrg1 / unm1 are the rounds' maps composed.
        mrg = mrg1 = unm1 = None
        TL, unm_pre = FN, 0
        for cur, randf in zip(*self.round_frames(F, self.randfs)):
            if mrg is not None:                                                 # the round before was not the last: its survivors become a sequence
                nxt = torch.empty(2, ne, TL, C, dtype=H16, device=self.dev)
                self._move(seq, sbs, met, mbs, mrg, nxt[0], TL * C, nxt[1], TL * C, TL, C, ne)
                seq, met, sbs, mbs = nxt[0], nxt[1], TL * C, TL * C
            a_pos, b_pos = self._positions(cur, N, randf, unm_pre)
            single = unm_pre == 0 and cur <= a["target_stride"]                # dst = the N tokens of frame randf, src = the rest: affine
            mrg, unm, Tn = self._match(met, mbs, TL, C, a_pos, a_pos.numel(), b_pos, b_pos.numel(), a["local_merge_ratio"],
                                       affine=(randf * N, N, randf * N) if single else None, ne=ne)
            if mrg1 is None:
                mrg1, unm1 = mrg, unm
            else:
                mrg1 = self._compose(mrg1, mrg, 0, Tn)                          # merged slot -> row of the joined input
                unm1 = self._compose(unm, unm1, 0, FN)                          # joined position -> slot of the current sequence
            unm_pre += Tn - b_pos.numel()                                       # ret_dict["unm_num"] = na - r
            TL = Tn
        if not a["merge_global"]:
            local = torch.empty(ne, TL, C, dtype=H16, device=self.dev)
            self._move(seq, sbs, None, 0, mrg, local, TL * C, None, 0, TL, C, ne)
            return Merged(local, TL * C, None), unm1, TL
        # ---- global merging (patch.py:59-82) against the block's bank.  The [local | bank] block is never copied together: the local tokens are
        # gathered straight into their slot of it, and the bank was written into its slot by the chunk that left it (`_next_block`: the next chunk's
        # frame count and coin were drawn at begin_step, so its layout is known).
        bank, bmet, home = self.banks.get(name), self._bank_met.get(name), self._home.pop(name, None)
        if bank is None:                                                        # patch.py:81-82: the first chunk seeds the bank with its local tokens
            tok, tmet = self._bank_slot(name, ne, TL, N, C)
            self._move(seq, sbs, met, mbs, mrg, tok, tok.stride(0), tmet, tmet.stride(0), TL, C, ne)
            self.banks[name], self._bank_met[name] = tok, tmet
            if self.trace is not None:
                self.trace.append(dict(name=name, F=F, unm=unm1, gather=mrg1, mrg1=mrg1, T=TL))
            return (Merged(tok, tok.stride(0), None) if lazy_merged else Merged(tok.contiguous(), TL * C, None)), unm1, TL
        if bank.shape[0] != ne:       # (a real exception: `python -O` strips asserts and a 2-entry gather would then read past a 1-entry bank)
            raise RuntimeError(f"VidToMe bank of block {name!r} was seeded with {bank.shape[0]} batch entr{'y' if bank.shape[0] == 1 else 'ies'}, this call "
                               f"carries {ne}: call reset_global_tokens() when switching between forward_many(cfg_pair=True) and the two-entry paths")
        Tb = bank.shape[1]
        src_len, loff, boff = self._slots(self.coin, TL, Tb)
        T = TL + Tb
        if home is not None and home[0].shape == (ne, T, C) and home[2:] == (TL, loff, boff) and bank.data_ptr() == home[0][:, boff:].data_ptr():
            cat, catm = home[0], home[1]                                        # the bank (and its metric) already sit in their slot
        else:
            cat, catm = torch.empty(ne, T, C, dtype=H16, device=self.dev), torch.empty(ne, T, C, dtype=H16, device=self.dev)
            self._move(bank, bank.stride(0), bmet, bmet.stride(0), None, cat[:, boff:], T * C, catm[:, boff:], T * C, Tb, C, ne)
        self._move(seq, sbs, met, mbs, mrg, cat[:, loff:], T * C, catm[:, loff:], T * C, TL, C, ne)
        mrg2, unm2, Tm = self._match(catm, T * C, T, C, self._range(0, src_len), src_len, self._range(src_len, T), T - src_len, a["global_merge_ratio"],
                                     affine=(src_len, 0, src_len), ne=ne)
        merged = self._merged(cat, T, mrg2, Tm, C, ne, lazy_merged)
        unm = self._compose(unm2, unm1, loff, FN)                               # 2s-unmerge then the randframe unmerges (func_warper(u_ls[::-1]))
        bmap = self._compose(mrg2, unm2[..., loff:], 0, TL)                     # bank <- u(merged_tokens), local part (patch.py:80)
        tok, tmet = self._bank_slot(name, ne, TL, N, C)
        self._move(cat, T * C, catm, T * C, bmap, tok, tok.stride(0), tmet, tmet.stride(0), TL, C, ne)
        self.banks[name], self._bank_met[name] = tok, tmet
        if self.trace is not None:
            self.trace.append(dict(name=name, F=F, unm=unm, mrg2=mrg2, mrg1=mrg1, T=Tm, loff=loff, boff=boff, TL=TL, bmap=bmap))
        return merged, unm, Tm
