// A stand-in for go-compression/raisin's compressor/huffman/huffman.go, written for the tests of go/overlay/split.py.
// It has the package-level layout the split reasons about -- Compress and Decompress next to the helpers they call
// and the Writer / Reader types that stay -- with small bodies of its own.
package huffman

import (
	"container/heap"
	"fmt"
	"io"
	"sort"
	"strconv"
	"strings"
)

type HuffmanTree interface {
	Freq() int
}

type HuffmanLeaf struct {
	freq  int
	value rune
}

type HuffmanNode struct {
	freq        int
	left, right HuffmanTree
}

func (l HuffmanLeaf) Freq() int { return l.freq }

func (n HuffmanNode) Freq() int { return n.freq }

type treeHeap []HuffmanTree

func (h treeHeap) Len() int            { return len(h) }
func (h treeHeap) Less(i, j int) bool  { return h[i].Freq() < h[j].Freq() }
func (h treeHeap) Swap(i, j int)       { h[i], h[j] = h[j], h[i] }
func (h *treeHeap) Push(x interface{}) { *h = append(*h, x.(HuffmanTree)) }
func (h *treeHeap) Pop() interface{} {
	old := *h
	x := old[len(old)-1]
	*h = old[:len(old)-1]
	return x
}

var header strings.Builder

func buildTree(freqs map[rune]int) HuffmanTree {
	keys := make([]int, 0, len(freqs))
	for r := range freqs {
		keys = append(keys, int(r))
	}
	sort.Ints(keys)
	var h treeHeap
	for _, k := range keys {
		h = append(h, HuffmanLeaf{freqs[rune(k)], rune(k)})
	}
	heap.Init(&h)
	for h.Len() > 1 {
		a, b := heap.Pop(&h).(HuffmanTree), heap.Pop(&h).(HuffmanTree)
		heap.Push(&h, HuffmanNode{a.Freq() + b.Freq(), a, b})
	}
	return heap.Pop(&h).(HuffmanTree)
}

func codes(t HuffmanTree, prefix string, into map[rune]string) {
	switch n := t.(type) {
	case HuffmanLeaf:
		into[n.value] = prefix
	case HuffmanNode:
		codes(n.left, prefix+"0", into)
		codes(n.right, prefix+"1", into)
	}
}

func encode(t HuffmanTree, input string) []byte {
	table := map[rune]string{}
	codes(t, "", table)
	var bits strings.Builder
	for _, r := range input {
		bits.WriteString(table[r])
	}
	return []byte(bits.String())
}

func decode(data []byte) []byte {
	parts := strings.SplitN(string(data), "\n", 2)
	if len(parts) != 2 {
		panic(fmt.Sprintf("huffman: no header in %d bytes", len(data)))
	}
	freqs := map[rune]int{}
	for _, f := range strings.Split(parts[0], "|") {
		if len(f) < 2 {
			continue
		}
		n, _ := strconv.Atoi(f[1:])
		freqs[rune(f[0])] = n
	}
	table := map[rune]string{}
	codes(buildTree(freqs), "", table)
	back := map[string]rune{}
	for r, c := range table {
		back[c] = r
	}
	var out strings.Builder
	cur := ""
	for _, b := range parts[1] {
		cur += string(b)
		if r, ok := back[cur]; ok {
			out.WriteRune(r)
			cur = ""
		}
	}
	return []byte(out.String())
}

// Compress writes the symbol counts, a newline, then the code bits.
func Compress(data []byte) []byte {
	freqs := map[rune]int{}
	for _, r := range string(data) {
		freqs[r]++
	}
	header.Reset()
	for r, n := range freqs {
		header.WriteString(fmt.Sprintf("%c%s|", r, strconv.Itoa(n)))
	}
	return append([]byte(header.String()+"\n"), encode(buildTree(freqs), string(data))...)
}

// Decompress is Compress's inverse.
func Decompress(data []byte) []byte {
	return decode(data)
}

type Writer struct {
	w    io.Writer
	data []byte
}

func NewWriter(w io.Writer) io.WriteCloser {
	return &Writer{w: w}
}

func (z *Writer) Write(p []byte) (int, error) {
	z.data = append(z.data, p...)
	return len(p), nil
}

func (z *Writer) Close() error {
	_, err := z.w.Write(Compress(z.data))
	return err
}

type Reader struct {
	r   io.Reader
	out []byte
}

func NewReader(r io.Reader) io.Reader {
	return &Reader{r: r}
}

func (z *Reader) Read(p []byte) (int, error) {
	if z.out == nil {
		var in strings.Builder
		if _, err := io.Copy(&in, z.r); err != nil {
			return 0, err
		}
		z.out = Decompress([]byte(in.String()))
	}
	if len(z.out) == 0 {
		return 0, io.EOF
	}
	n := copy(p, z.out)
	z.out = z.out[n:]
	return n, nil
}
