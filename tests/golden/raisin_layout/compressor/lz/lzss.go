// A stand-in for go-compression/raisin's compressor/lz/lzss.go, written for the tests of go/overlay/split.py.
// It has the package-level layout the split reasons about -- the same exported and unexported function names,
// an aliased import, `sync` used by CompressAsync and compressorWorkerAsync alone, compressorWorker called by
// CompressRecursive as well, doc comments above moved functions -- with small bodies of its own.
package lz

import (
	"bytes"
	"fmt"
	pb "github.com/cheggaaa/pb/v3"
	"io"
	"strconv"
	"sync"
)

const (
	Opening   = '<'
	Closing   = '>'
	Separator = ','
)

const MinimumSizeOfReference int = -1

type Reference struct {
	Value    []byte
	IsRef    bool
	Pointer  int
	Length   int
	Position int
}

type Writer struct {
	w      io.Writer
	window int
	data   []byte
}

const DefaultWindowSize = 4096

func NewWriter(w io.Writer) io.WriteCloser {
	z, _ := NewWriterLevel(w, DefaultWindowSize)
	return z
}

func NewWriterLevel(w io.Writer, level int) (*Writer, error) {
	if level < 1 {
		return nil, fmt.Errorf("lz: window %d is not positive", level)
	}
	return &Writer{w: w, window: level}, nil
}

func (z *Writer) Write(p []byte) (int, error) {
	z.data = append(z.data, p...)
	return len(p), nil
}

func (z *Writer) Close() error {
	_, err := z.w.Write(CompressAsync(z.data, false, z.window))
	return err
}

type Reader struct {
	r    io.Reader
	out  []byte
	done bool
}

func (z *Reader) Read(p []byte) (int, error) {
	if !z.done {
		var in bytes.Buffer
		if _, err := in.ReadFrom(z.r); err != nil {
			return 0, err
		}
		z.out, z.done = Decompress(in.Bytes(), false), true
	}
	if len(z.out) == 0 {
		return 0, io.EOF
	}
	n := copy(p, z.out)
	z.out = z.out[n:]
	return n, nil
}

func NewReader(r io.Reader) io.Reader {
	return &Reader{r: r}
}

// CompressAsync searches every position at once (one goroutine each),
// then emits the references in order.
func CompressAsync(data []byte, progress bool, window int) []byte {
	var bar *pb.ProgressBar
	if progress {
		bar = pb.StartNew(len(data))
	}
	refs := make([]Reference, len(data))
	var wg sync.WaitGroup
	for i := range data {
		lo := i - window
		if lo < 0 {
			lo = 0
		}
		wg.Add(1)
		go compressorWorkerAsync(&wg, &refs[i], data[lo:i], data[i:], bar)
	}
	wg.Wait()
	out := []byte{}
	for i := 0; i < len(refs); {
		if refs[i].IsRef {
			out = append(out, getEncoding(refs[i].Pointer, refs[i].Length)...)
			i += refs[i].Length
		} else {
			out = append(out, EncodeOpeningSymbols(data[i:i+1])...)
			i++
		}
	}
	return out
}

func compressorWorkerAsync(wg *sync.WaitGroup, slot *Reference, window []byte, rest []byte, bar *pb.ProgressBar) {
	defer wg.Done()
	*slot = compressorWorker(window, rest, bar)
}

func compressorWorker(window []byte, rest []byte, bar *pb.ProgressBar) Reference {
	if bar != nil {
		bar.Increment()
	}
	best := Reference{}
	for n := 1; n <= len(rest); n++ {
		at, ok := FindReverseSlice(window, rest[:n])
		if !ok {
			break
		}
		best = Reference{IsRef: true, Pointer: len(window) - at, Length: n}
	}
	return best
}

// CompressRecursive is the serial form of CompressAsync.
func CompressRecursive(data []byte, _ bool, window int) []byte {
	out := []byte{}
	for i := 0; i < len(data); {
		lo := i - window
		if lo < 0 {
			lo = 0
		}
		if ref := compressorWorker(data[lo:i], data[i:], nil); ref.IsRef {
			out = append(out, getEncoding(ref.Pointer, ref.Length)...)
			i += ref.Length
			continue
		}
		out = append(out, EncodeOpeningSymbols(data[i:i+1])...)
		i++
	}
	return out
}

// Compress is the single-thread encoder.
func Compress(data []byte, progress bool, window int) []byte {
	var bar *pb.ProgressBar
	if progress {
		bar = pb.StartNew(len(data))
	}
	out := []byte{}
	for i := 0; i < len(data); i++ {
		if bar != nil {
			bar.Increment()
		}
		if at, ok := FindReverse(data[:i], data[i]); ok && MinimumSizeOfReference < 0 {
			out = append(out, getEncoding(i-at, 1)...)
			continue
		}
		out = append(out, EncodeOpeningSymbols(data[i:i+1])...)
	}
	_ = strconv.Itoa(len(out))
	return out
}

func getEncoding(pointer int, length int) []byte {
	return []byte(string(Opening) + strconv.Itoa(pointer) + string(Separator) + strconv.Itoa(length) + string(Closing))
}

// Decompress expands every <pointer,length> token.
func Decompress(data []byte, progress bool) []byte {
	out := []byte{}
	for i := 0; i < len(data); i++ {
		if data[i] != Opening {
			out = append(out, data[i])
			continue
		}
		j := i + 1
		for j < len(data) && data[j] != Closing {
			j++
		}
		parts := bytes.Split(data[i+1:j], []byte{Separator})
		p, _ := strconv.Atoi(string(parts[0]))
		n, _ := strconv.Atoi(string(parts[1]))
		for k := 0; k < n; k++ {
			out = append(out, out[len(out)-p])
		}
		i = j
	}
	return DecodeOpeningSymbols(out)
}

const EncodedOpening = 0xff
const EscapeByte = 0x5c

func EncodeOpeningSymbols(b []byte) []byte {
	out := make([]byte, 0, len(b))
	for _, c := range b {
		if c == Opening || c == EscapeByte {
			out = append(out, EscapeByte)
		}
		out = append(out, c)
	}
	return out
}

func DecodeOpeningSymbols(b []byte) []byte {
	out := make([]byte, 0, len(b))
	for i := 0; i < len(b); i++ {
		if b[i] == EscapeByte && i+1 < len(b) {
			i++
		}
		out = append(out, b[i])
	}
	return out
}

func FindReverseSlice(haystack []byte, needle []byte) (int, bool) {
	at := bytes.LastIndex(haystack, needle)
	return at, at >= 0
}

func FindReverse(s []byte, v byte) (int, bool) {
	for i := len(s) - 1; i >= 0; i-- {
		if s[i] == v {
			return i, true
		}
	}
	return -1, false
}
