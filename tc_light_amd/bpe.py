"""CLIP's byte-level BPE from `vocab.json` + `merges.txt`, with the interface text.py and clip.py program against: `tok(txt, truncation=False,
add_special_tokens=False)["input_ids"]`, `.bos_token_id`, `.eos_token_id`, `.model_max_length`.

A restatement, from the two file formats, of what `transformers.CLIPTokenizer` computes when `ftfy` is not installed (the reference environment; ftfy's
text fixing is not done here): the text is cut at literal `<|startoftext|>` / `<|endoftext|>`, which become their ids; every other stretch is NFC
normalised, its whitespace runs become one space, it is lower-cased and cut into words by the pattern below (contractions, letter runs, single
digits, runs of anything else; whitespace separates and is dropped).  A word's UTF-8 bytes are written as the 256 printable stand-in characters of
GPT-2's table, the last one gets `</w>`, and adjacent symbols are merged, the pair of lowest rank in merges.txt first (the leftmost one among equals),
until no adjacent pair is a merge.  A start symbol the vocabulary lacks is the unknown token, `<|endoftext|>`.  Words are cached.
Pinned against `transformers.CLIPTokenizer` on a synthetic vocabulary by tests/test_text_host_cpu.py.
"""
import json
import os
import unicodedata

import regex

BOS, EOS = "<|startoftext|>", "<|endoftext|>"
# CLIP's split pattern, <\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+, without its first two alternatives: a
# literal special token never reaches it (encode cuts the raw text at them), and one that appears only through lower-casing ("<|ENDOFTEXT|>") is cut
# into "<|", "endoftext", "|>" by the byte-level stage of transformers' tokenizer -- which is what the remaining alternatives give
_WORDS = regex.compile(r"'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+")
_SPACES = regex.compile(r"\s+")
_SPECIALS = regex.compile(r"(<\|startoftext\|>|<\|endoftext\|>)")


def byte_symbols():
    """byte -> its stand-in character: the printable Latin-1 bytes are themselves, the other 68 are U+0100 onwards in byte order."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    table, n = {b: chr(b) for b in keep}, 0
    for b in range(256):
        if b not in table:
            table[b] = chr(256 + n)
            n += 1
    return table


class CLIPBPE:
    def __init__(self, vocab_json, merges_txt, model_max_length=77):
        with open(vocab_json, encoding="utf-8") as f:
            self.vocab = json.load(f)
        missing = [t for t in (BOS, EOS) if t not in self.vocab]
        if missing:
            raise ValueError(f"{vocab_json!r} lacks {missing}: not a CLIP vocabulary")
        self.bos_token_id, self.eos_token_id = int(self.vocab[BOS]), int(self.vocab[EOS])
        self.unk_token_id = self.eos_token_id
        self.model_max_length = int(model_max_length)
        self.merges = {}                                                 # (left id, right id) -> (rank, merged id)
        with open(merges_txt, encoding="utf-8") as f:
            lines = f.read().split("\n")
        for ln in lines:
            if not ln.strip() or ln.startswith("#version"):
                continue
            parts = ln.split(" ")
            if len(parts) != 2:
                raise ValueError(f"{merges_txt!r}: a merge is two symbols separated by one space, got {ln!r}")
            a, b = parts
            lost = [s for s in (a, b, a + b) if s not in self.vocab]
            if lost:
                raise ValueError(f"{merges_txt!r}: merge {ln!r} names {lost[0]!r}, which {os.path.basename(vocab_json)} does not hold")
            self.merges.setdefault((self.vocab[a], self.vocab[b]), (len(self.merges), self.vocab[a + b]))
        self._bytes = byte_symbols()
        self._cache = {}

    @classmethod
    def from_dir(cls, d):
        """The tokenizer of directory `d` or of `d/tokenizer` (vocab.json + merges.txt; model_max_length from tokenizer_config.json when there is
        one, else 77), or None when neither holds both files."""
        for p in (d, os.path.join(d, "tokenizer") if d else None):
            if p and os.path.isfile(os.path.join(p, "vocab.json")) and os.path.isfile(os.path.join(p, "merges.txt")):
                length, cfg = 77, os.path.join(p, "tokenizer_config.json")
                if os.path.isfile(cfg):
                    with open(cfg, encoding="utf-8") as f:
                        length = json.load(f).get("model_max_length", 77)
                return cls(os.path.join(p, "vocab.json"), os.path.join(p, "merges.txt"), length)
        return None

    def _word(self, word):
        ids = self._cache.get(word)
        if ids is not None:
            return ids
        sym = [self._bytes[b] for b in word.encode("utf-8")]
        sym[-1] += "</w>"
        ids = [self.vocab.get(s, self.unk_token_id) for s in sym]
        while len(ids) > 1:
            best = min(((self.merges.get((ids[i], ids[i + 1]), (len(self.merges),))[0], i) for i in range(len(ids) - 1)))
            if best[0] == len(self.merges):
                break
            i = best[1]
            ids[i:i + 2] = [self.merges[ids[i], ids[i + 1]][1]]
        self._cache[word] = ids
        return ids

    def encode(self, txt):
        """The ids of `txt`, without BOS / EOS and untruncated."""
        out = []
        for k, part in enumerate(_SPECIALS.split(txt)):
            if k % 2:                                                    # a literal special token
                out.append(self.vocab[part])
                continue
            part = _SPACES.sub(" ", unicodedata.normalize("NFC", part)).strip().lower()
            for w in _WORDS.findall(part):
                out.extend(self._word(w))
        return out

    def __call__(self, txt, truncation=False, add_special_tokens=False):
        if truncation or add_special_tokens:
            raise ValueError("CLIPBPE gives the bare, untruncated ids: the callers lay out BOS / EOS and the chunks (truncation=False, "
                             "add_special_tokens=False)")
        return {"input_ids": self.encode(txt)}
