------------------------------ MODULE refuse_symmetry ------------------------------
(* Refused: SYMMETRY stays unsupported for compiled PlusCal programs. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm refuse_symmetry
variables x = 0, y = 0;

process P \in 1..2
begin
  a: x := x + 1;
  b: y := y + x;
end process

end algorithm *)

Perms == Permutations(1..2)
=============================================================================
