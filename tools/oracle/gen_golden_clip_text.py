"""Data for the CLIP text side (patchioner_amd/clip_text.py).  Run in the build container only:

    python tools/oracle/gen_golden_clip_text.py [merges] [tokenize] [tower]

merges    patchioner_amd/assets/clip_bpe_merge_splits.txt: the merge list of the reference's BPE vocabulary file
          (P/src/clip/bpe_simple_vocab_16e6.txt.gz, the rows clip's SimpleTokenizer keeps) as plain text: for merge r, which
          produces vocabulary entry 512 + r, the byte length of its left part (the pair of ids follows from the decode
          table, clip_text.merges_from_splits; checked here against the list).  Data only, derived as the decode table was
          (tools/oracle/gen_golden.py).
tokenize  tests/golden/clip_tokenize.npz: ~200 sentences and the ids the REFERENCE's SimpleTokenizer.encode gives them.
          ``ftfy`` is not installed here, so it is stubbed with the identity -- which is what ``ftfy.fix_text`` is for every
          sentence of the set: well-formed NFC text without curly quotes, mojibake, HTML entities, ligatures or full-width
          forms (each sentence is checked against the product's own fix_text, which must leave it unchanged).
tower     tests/golden/clip_text_hf.npz: transformers.CLIPTextModelWithProjection (an independent implementation of the
          OpenAI text tower, eager attention, fp32 CPU, eos_token_id = 49407) carrying weights.synth_clip_text for
          ViT-B/16 (512 x 8) and ViT-L/14 (768 x 12) at depth 12, on clip.tokenize rows of a caption set.
"""
import gzip
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import refshim  # noqa: E402
from patchioner_amd import clip_text as CT  # noqa: E402
from patchioner_amd import weights as W  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CLIP_DIR = os.path.join(refshim.REF_SRC, "clip")
torch.set_grad_enabled(False)

SEED_B16, SEED_L14 = 501, 502


def ref_tokenizer():
    if "ftfy" not in sys.modules:
        sys.modules["ftfy"] = types.SimpleNamespace(fix_text=lambda s: s)     # identity: see the header
    spec = importlib.util.spec_from_file_location("ref_simple_tokenizer", os.path.join(CLIP_DIR, "simple_tokenizer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SimpleTokenizer(os.path.join(CLIP_DIR, "bpe_simple_vocab_16e6.txt.gz"))


def gen_merges(tok):
    lines = gzip.open(os.path.join(CLIP_DIR, "bpe_simple_vocab_16e6.txt.gz")).read().decode("utf-8").split("\n")
    merges = [tuple(m.split()) for m in lines[1:49152 - 256 - 2 + 1]]
    arr = np.zeros((len(merges), 2), np.int64)
    splits = []
    for r, (a, b) in enumerate(merges):
        arr[r] = tok.encoder[a], tok.encoder[b]
        assert tok.encoder[a + b] == 512 + r
        splits.append(len(bytes(tok.byte_decoder[c] for c in a)))
    from patchioner_amd.tokenizer import ClipDetokenizer
    assert np.array_equal(CT.merges_from_splits(ClipDetokenizer().table, splits), arr)
    path = os.path.join(ROOT, "patchioner_amd", "assets", "clip_bpe_merge_splits.txt")
    with open(path, "w", encoding="ascii") as f:
        f.write("# CLIP BPE merges: byte length of the left part of merge r (vocabulary entry 512 + r), r = 0, 1, ...; "
                "see patchioner_amd/clip_text.py\n")
        for i in range(0, len(splits), 40):
            f.write(" ".join(str(p) for p in splits[i:i + 40]) + "\n")
    print("wrote %s (%d merges, %.1f KB)" % (path, len(splits), os.path.getsize(path) / 1024))


def sentences():
    rng = np.random.RandomState(17)
    adj = ["small", "large", "red", "wooden", "happy", "old", "shiny", "crowded", "empty", "striped", "fluffy", "brightly-lit"]
    noun = ["dog", "cat", "man", "woman", "giraffe", "skateboarder", "pizza", "bus", "kitchen", "surfboard", "zebra", "laptop",
            "bathroom", "frisbee", "elephant", "train", "umbrella", "sandwich", "bicycle", "teddy bear"]
    verb = ["sitting", "standing", "riding", "eating", "holding", "parked", "walking", "laying", "flying", "looking"]
    prep = ["on", "next to", "in front of", "near", "under", "beside", "inside", "across"]
    out = []
    for i in range(130):
        s = "%s %s %s %s %s %s" % (rng.choice(["A", "An", "The", "Two", "a", "Several"]), rng.choice(adj), rng.choice(noun),
                                   rng.choice(verb), rng.choice(prep), "the " + rng.choice(noun))
        if i % 3 == 0:
            s += " with a %s %s" % (rng.choice(adj), rng.choice(noun))
        s += rng.choice([".", "", " .", "!", "...", ",", " ?"])
        if i % 11 == 0:
            s = s.upper()
        out.append(s)
    out += [
        "Hello, world!!", "what?!...", "(a dog) [on] {grass}", "e-mail & co.", "50% off -- now!", "#hashtag @user",
        "C++ / C# / F#", "a.b.c", "x=y+z*2", "semi;colon:colon", "~tilde^caret|pipe\\back", "quotes \"double\" and 'single'",
        "It's a dog's life", "they're here", "we've been", "I'm fine", "you'll see", "he'd go", "don't", "CAN'T STOP",
        "rock 'n' roll", "'s", "'tis the season", "o'clock", "the '90s",
        "2 dogs and 13 cats in 1999", "3.14159", "room 101b", "1st 2nd 3rd 4th", "0", "1234567890", "phone: 555-0199",
        "café crème", "naïve façade", "Straße", "Ελληνικά λέξεις", "Привет мир", "日本語のテキスト", "한국어 문장", "مرحبا بالعالم",
        "emoji 🐶🐱 pets", "Zürich über alles", "ñandú", "São Paulo", "œuvre", "Ångström", "١٢٣ arabic digits", "Ⅻ roman",
        "", "   ", "\t\n", "  multiple   spaces\tand\ttabs\nnewlines  ", "a", "A", ".", "!!!",
        "a <|startoftext|> b", "x<|endoftext|>y", "supercalifragilisticexpialidocious", "antidisestablishmentarianism",
        "http://example.com/path?q=1", "snake_case_words and camelCaseWords", "mixed123letters456",
    ]
    out.append(" ".join(["dog"] * 75))        # 75 + SOT + EOT = 77: the boundary row
    out.append(" ".join(["dog"] * 76))        # 78: clip.tokenize raises, truncate keeps EOT last
    for s in out:
        assert CT.fix_text(s) == s, s
    return out


def gen_tokenize(tok):
    sents = sentences()
    ids = [tok.encode(s) for s in sents]
    offs = np.zeros(len(ids) + 1, np.int64)
    offs[1:] = np.cumsum([len(i) for i in ids])
    flat = np.asarray([t for row in ids for t in row], np.int32)
    path = os.path.join(OUT, "clip_tokenize.npz")
    np.savez_compressed(path, strings_json=np.frombuffer(json.dumps(sents).encode(), np.uint8), ids=flat, offsets=offs)
    print("wrote %s (%d sentences)" % (path, len(sents)))


def hf_text_model(w, heads):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    V, Wd = w["token_embedding.weight"].shape
    C, E = w["positional_embedding"].shape[0], w["text_projection"].shape[1]
    depth = 1 + max(int(k.split(".")[2]) for k in w if k.startswith("transformer.resblocks."))
    cfg = CLIPTextConfig(vocab_size=V, hidden_size=Wd, intermediate_size=4 * Wd, num_hidden_layers=depth, num_attention_heads=heads,
                         max_position_embeddings=C, projection_dim=E, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                         eos_token_id=49407, bos_token_id=49406, pad_token_id=0, attn_implementation="eager")
    m = CLIPTextModelWithProjection(cfg).eval()
    sd = {"text_model.embeddings.token_embedding.weight": w["token_embedding.weight"],
          "text_model.embeddings.position_embedding.weight": w["positional_embedding"],
          "text_model.final_layer_norm.weight": w["ln_final.weight"], "text_model.final_layer_norm.bias": w["ln_final.bias"],
          "text_projection.weight": w["text_projection"].t().contiguous()}
    for i in range(depth):
        s, t = "transformer.resblocks.%d." % i, "text_model.encoder.layers.%d." % i
        for nm, ww, bb in zip(("q_proj", "k_proj", "v_proj"), w[s + "attn.in_proj_weight"].chunk(3, 0), w[s + "attn.in_proj_bias"].chunk(3, 0)):
            sd[t + "self_attn.%s.weight" % nm], sd[t + "self_attn.%s.bias" % nm] = ww, bb
        sd[t + "self_attn.out_proj.weight"], sd[t + "self_attn.out_proj.bias"] = w[s + "attn.out_proj.weight"], w[s + "attn.out_proj.bias"]
        sd[t + "layer_norm1.weight"], sd[t + "layer_norm1.bias"] = w[s + "ln_1.weight"], w[s + "ln_1.bias"]
        sd[t + "layer_norm2.weight"], sd[t + "layer_norm2.bias"] = w[s + "ln_2.weight"], w[s + "ln_2.bias"]
        sd[t + "mlp.fc1.weight"], sd[t + "mlp.fc1.bias"] = w[s + "mlp.c_fc.weight"], w[s + "mlp.c_fc.bias"]
        sd[t + "mlp.fc2.weight"], sd[t + "mlp.fc2.bias"] = w[s + "mlp.c_proj.weight"], w[s + "mlp.c_proj.bias"]
    missing, unexpected = m.load_state_dict(sd, strict=False)
    missing = [k for k in missing if "position_ids" not in k]
    assert not missing and not unexpected, (missing, unexpected)
    return m


TOWER_TEXTS = ["A dog sitting on a red couch.", "", "two zebras", "A man riding a wave on top of a surfboard.",
               "a kitchen with wooden cabinets, a white stove and a window over the sink", "It's a cat!",
               " ".join(["dog"] * 75), "café crème on the table"]


def gen_tower():
    ids = CT.tokenize(TOWER_TEXTS)
    arrs = {"ids": ids.numpy().astype(np.int32), "texts_json": np.frombuffer(json.dumps(TOWER_TEXTS).encode(), np.uint8)}
    for tag, name, seed, heads in (("b16", "ViT-B/16", SEED_B16, 8), ("l14", "ViT-L/14", SEED_L14, 12)):
        m = hf_text_model(W.synth_clip_text(seed, name), heads)
        arrs["%s_feats" % tag] = m(input_ids=ids).text_embeds.numpy()
    path = os.path.join(OUT, "clip_text_hf.npz")
    np.savez_compressed(path, **arrs)
    print("wrote %s" % path)


def main():
    only = set(sys.argv[1:])
    want = lambda n: not only or n in only  # noqa: E731
    tok = ref_tokenizer() if (want("merges") or want("tokenize")) else None
    if want("merges"):
        gen_merges(tok)
    if want("tokenize"):
        gen_tokenize(tok)
    if want("tower"):
        gen_tower()


if __name__ == "__main__":
    main()
