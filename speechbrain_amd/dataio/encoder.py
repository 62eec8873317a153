"""speechbrain.dataio.encoder mirror: the part of CTCTextEncoder (dataio/encoder.py:1057-1195) an EncoderASR needs --
the label <-> index maps, decode_ndim, the blank index and loading of the reference's label file (the Python-literal
format of CategoricalEncoder.save / load, :607-640,776-820)."""
import ast

DEFAULT_BLANK = "<blank>"


class CTCTextEncoder:
    VALUE_SEPARATOR = " => "
    EXTRAS_SEPARATOR = "================\n"

    def __init__(self, starting_index=0, **special_labels):
        self.lab2ind = {}
        self.ind2lab = {}
        self.starting_index = starting_index
        if "blank_label" in special_labels:
            self.insert_blank(index=special_labels["blank_label"])
        if "unk_label" in special_labels:
            self.unk_label = special_labels["unk_label"]

    def __len__(self):
        return len(self.lab2ind)

    def insert_blank(self, blank_label=DEFAULT_BLANK, index=0):
        if blank_label in self.lab2ind:
            raise KeyError(f"Label already present: {blank_label}")
        shifted = {lab: (i + 1 if i >= index else i) for lab, i in self.lab2ind.items()}
        shifted[blank_label] = index
        self.lab2ind = shifted
        self.ind2lab = {i: lab for lab, i in shifted.items()}
        self.blank_label = blank_label

    def get_blank_index(self):
        if not hasattr(self, "blank_label"):
            raise RuntimeError("Blank label is not set!")
        return self.lab2ind[self.blank_label]

    def decode_ndim(self, x):
        """Nested iterable (or one element) of indices -> the same nesting of labels (:565-590)."""
        if not self.lab2ind:
            raise RuntimeError("CTCTextEncoder is empty")
        try:
            return [self.decode_ndim(sub) for sub in x]
        except TypeError:
            return self.ind2lab[int(x)]

    def encode_sequence(self, sequence):
        return [self.lab2ind[lab] if lab in self.lab2ind or not hasattr(self, "unk_label") else
                self.lab2ind[self.unk_label] for lab in sequence]

    def load(self, path):
        lab2ind, ind2lab, extras = {}, {}, {}
        with open(path, encoding="utf-8") as f:
            for line in f:
                if line == self.EXTRAS_SEPARATOR:
                    break
                literal, ind = line.strip().split(self.VALUE_SEPARATOR, maxsplit=1)
                label = ast.literal_eval(literal)
                lab2ind[label], ind2lab[int(ind)] = int(ind), label
            for line in f:
                key, value = line.strip().split(self.VALUE_SEPARATOR, maxsplit=1)
                extras[ast.literal_eval(key)] = ast.literal_eval(value)
        self.lab2ind, self.ind2lab = lab2ind, ind2lab
        if "unk_label" in extras:
            self.unk_label = extras["unk_label"]
        if "blank_label" in extras:
            self.blank_label = extras["blank_label"]
        self.starting_index = extras.get("starting_index", 0)

    def _load(self, path):  # Pretrainer.load_collected calls a loadable object's _load
        self.load(path)

    def save(self, path):
        extras = {"starting_index": self.starting_index}
        if hasattr(self, "unk_label"):
            extras["unk_label"] = self.unk_label
        if hasattr(self, "blank_label"):
            extras["blank_label"] = self.blank_label
        with open(path, "w", encoding="utf-8") as f:
            for label, ind in self.lab2ind.items():
                f.write(repr(label) + self.VALUE_SEPARATOR + str(ind) + "\n")
            f.write(self.EXTRAS_SEPARATOR)
            for key, value in extras.items():
                f.write(repr(key) + self.VALUE_SEPARATOR + repr(value) + "\n")
